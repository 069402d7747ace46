"""Fused clip + Adam step on a torch.optim.Adam instance (train_seg_gan.py:211-215,229-233), and the same for the
torch.optim.SGD that the stage-1 config can ask for instead (train.py:292-294).

The training loop receives stock torch.optim.Adam objects from its caller; this helper runs
the same update as `clip_gradient(opt, c); opt.step()` in ONE multi-tensor HIP launch while
keeping the optimizer's own state (`exp_avg`, `exp_avg_sq`, `step`) authoritative, so
optimizer.state_dict() stays interchangeable with the reference's.  clip_sgd_step does the same with SGD's `momentum_buffer`."""
import math

import torch

from . import _lib, ops
from ._lib import call, ptr, stream_ptr

ADAM_CHUNK = 4096
_PLAN_CACHE = {}


def _supported(opt):
    if type(opt) is not torch.optim.Adam:
        return False
    for g in opt.param_groups:
        if g.get('amsgrad') or g.get('maximize') or g.get('capturable') or g.get('differentiable'):
            return False
        if isinstance(g['lr'], torch.Tensor):
            return False
    return True


def _build_plan(ptrs, sizes, device):
    """Device-side launch plan of the multi-tensor kernels: 4 pointers and one size per tensor, one block per 4096-element chunk."""
    blk_t, blk_c = [], []
    for t, n in enumerate(sizes):
        for c in range((n + ADAM_CHUNK - 1) // ADAM_CHUNK):
            blk_t.append(t); blk_c.append(c)
    return (torch.tensor(ptrs, dtype=torch.int64).to(device), torch.tensor(sizes, dtype=torch.int64).to(device),
            torch.tensor(blk_t, dtype=torch.int32).to(device), torch.tensor(blk_c, dtype=torch.int32).to(device), len(blk_t))


def _cached_plan(key, ptrs, sizes, device):
    """The plan under `key`.  The cache holds no reference to the tensors and the allocator may hand their addresses to
    tensors of another size, so every key carries every numel next to the pointers: a plan is only reused for the launch
    it was built for."""
    hit = _PLAN_CACHE.get(key)
    if hit is not None:
        return hit
    plan = _build_plan(ptrs, sizes, device)
    if len(_PLAN_CACHE) > 64:
        _PLAN_CACHE.clear()
    _PLAN_CACHE[key] = plan
    return plan


def _plan(params, states, device):
    ptrs, sizes = [], []
    for p, s in zip(params, states):
        ptrs += [p.data_ptr(), p.grad.data_ptr(), s['exp_avg'].data_ptr(), s['exp_avg_sq'].data_ptr()]
        sizes.append(p.numel())
    return _cached_plan((tuple(ptrs), tuple(sizes)), ptrs, sizes, device)


def _clamp_plan(params, device):
    ptrs, sizes = [], []
    for p in params:
        ptrs += [p.data_ptr(), 0, 0, 0]
        sizes.append(p.numel())
    return _cached_plan(('clampw', tuple(ptrs), tuple(sizes)), ptrs, sizes, device)


def clip_adam_step(optimizer, grad_clip=None):
    """Equivalent of `clip_gradient(optimizer, grad_clip); optimizer.step()`."""
    if not _supported(optimizer):
        raise NotImplementedError('clip_adam_step supports plain torch.optim.Adam (no amsgrad/maximize/capturable)')
    for group in optimizer.param_groups:
        params = [p for p in group['params'] if p.grad is not None]
        if not params:
            continue
        states = []
        for p in params:
            _lib.require_gpu(p)
            if not (p.is_contiguous() and p.grad.is_contiguous() and p.dtype == torch.float32):
                raise ValueError('clip_adam_step: parameters and grads must be contiguous fp32')
            st = optimizer.state[p]
            if len(st) == 0:                    # same lazy init as torch.optim.Adam
                st['step'] = torch.tensor(0.0, dtype=torch.float32)
                st['exp_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)
            states.append(st)
        steps = {float(st['step']) for st in states}
        if len(steps) != 1:
            raise NotImplementedError('clip_adam_step: parameters with different step counts in one group')
        step = steps.pop() + 1.0
        for st in states:
            st['step'] += 1
        beta1, beta2 = group['betas']
        bc1 = 1.0 - beta1 ** step
        bc2_sqrt = math.sqrt(1.0 - beta2 ** step)
        ptrs, sizes, blk_t, blk_c, nblk = _plan(params, states, params[0].device)
        call('ssg_clamp_adam_multi_f32', ptr(ptrs), ptr(sizes), ptr(blk_t), ptr(blk_c), nblk,
             float(grad_clip) if grad_clip else 0.0, float(group['lr']), float(beta1), float(beta2), float(group['eps']),
             float(group['weight_decay']), bc1, bc2_sqrt, stream_ptr())
    ops.bump_weight_epoch()


def _supported_sgd(opt):
    if type(opt) is not torch.optim.SGD:
        return False
    for g in opt.param_groups:
        if g.get('maximize') or g.get('differentiable'):
            return False
        if isinstance(g['lr'], torch.Tensor):
            return False
    return True


def _sgd_plan(params, bufs, first, device):
    """Record {param, grad, momentum_buffer or 0, first-step flag}: the flag travels in the pointer array, so it is part of
    the key.  A tensor's second step has its first step's four addresses and another flag."""
    ptrs, sizes = [], []
    for p, b, f in zip(params, bufs, first):
        ptrs += [p.data_ptr(), p.grad.data_ptr(), b.data_ptr() if b is not None else 0, int(bool(f))]
        sizes.append(p.numel())
    return _cached_plan(('sgd', tuple(ptrs), tuple(sizes)), ptrs, sizes, device)


def clip_sgd_step(optimizer, grad_clip=None):
    """Equivalent of `clip_gradient(optimizer, grad_clip); optimizer.step()` for torch.optim.SGD, one launch per group."""
    if not _supported_sgd(optimizer):
        raise NotImplementedError('clip_sgd_step supports plain torch.optim.SGD (no maximize/differentiable/tensor lr)')
    for group in optimizer.param_groups:
        params = [p for p in group['params'] if p.grad is not None]
        if not params:
            continue
        momentum = float(group['momentum'])
        bufs, first = [], []
        for p in params:
            _lib.require_gpu(p)
            if not (p.is_contiguous() and p.grad.is_contiguous() and p.dtype == torch.float32 and p.grad.dtype == torch.float32):
                raise ValueError('clip_sgd_step: parameters and grads must be contiguous fp32')
            buf = optimizer.state[p].get('momentum_buffer') if momentum != 0 else None
            first.append(momentum != 0 and buf is None)
            if first[-1]:                       # torch.optim.SGD clones the gradient here; the kernel writes every element
                buf = torch.empty_like(p, memory_format=torch.contiguous_format)
            elif buf is not None and not (buf.is_contiguous() and buf.dtype == torch.float32 and buf.device == p.device
                                          and buf.numel() == p.numel()):
                raise ValueError('clip_sgd_step: momentum_buffer must be a contiguous fp32 tensor of the parameter\'s size and device')
            bufs.append(buf)
        ptrs, sizes, blk_t, blk_c, nblk = _sgd_plan(params, bufs, first, params[0].device)
        call('ssg_clamp_sgd_multi_f32', ptr(ptrs), ptr(sizes), ptr(blk_t), ptr(blk_c), nblk,
             float(grad_clip) if grad_clip else 0.0, float(group['lr']), momentum, float(group['dampening']),
             float(group['weight_decay']), int(bool(group['nesterov'])), stream_ptr())
        for p, buf, f in zip(params, bufs, first):
            if f:
                optimizer.state[p]['momentum_buffer'] = buf
    optimizer._opt_called = True             # what lr_scheduler's wrapper of step() records: scheduler.step() does not warn
    ops.bump_weight_epoch()


def clamp_parameters_(params, clip):
    """`for p in params: p.data.clamp_(-clip, clip)` (train.py:111-112) in one multi-tensor launch."""
    params = [p for p in params]
    if not params:
        return
    for p in params:
        _lib.require_gpu(p)
        if not p.is_contiguous() or p.dtype != torch.float32:
            raise ValueError('clamp_parameters_: parameters must be contiguous fp32')
    ptrs, sizes, blk_t, blk_c, nblk = _clamp_plan(params, params[0].device)
    call('ssg_clamp_multi_f32', ptr(ptrs), ptr(sizes), ptr(blk_t), ptr(blk_c), nblk, 0, -float(clip), float(clip), stream_ptr())
    ops.bump_weight_epoch()              # packed-weight caches must see the clamped values
