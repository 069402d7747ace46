"""The fused clip + SGD step (csrc/pointwise.hip clamp_sgd_kernel, optim.clip_sgd_step) and its wiring into both trainers.

Two oracles, both on the CPU from the same fp32 values: an fp64 restatement of torch.optim.SGD's formulas (_sgd64), and
stock torch.optim.SGD on fp32 copies after grad.clamp_.  The gate is the project's "no worse than twice the fp32 path's own
error" rule (tests/test_split_gpu.py): over the parameters of the optimizer, and over its momentum buffers,

    max |GPU - fp64|  <=  2 * max |CPU fp32 torch - fp64|  +  one fp32 ulp of the largest magnitude compared.

The maxima run over every tensor of the optimizer together, not per tensor: the kernel rounds as often as torch does (each
add(x, alpha=a) is one FMA) but not identically, so on a 1-element tensor either side can land on the fp64 value by chance
while the other is half an ulp away; over the ~37000 elements that one launch updates the two maxima are comparable."""
import copy
import itertools
import warnings

import numpy as np
import pytest
import torch

from test_step_tail_gpu import _Carved, _bits, _gen

pytestmark = pytest.mark.gpu

SIZES = (1, 3, 4095, 4096, 4097, 3 * 4096 + 5)       # the edges of the 4096-element chunks and of the float4 body
ODD_SIZE = 4099                                       # the parameter 4 bytes past a 16-byte boundary: two chunks on the scalar loop
GROUPS = (((0, 2, 4, 6, 7), 5e-2), ((1, 3, 5, 8), 1e-2))                # parameter indices and lr of the two groups
SKIP_ONCE, SKIP_TWICE = 4, 5                          # no gradient on step 2 / on steps 1 and 2 (first momentum step on step 3)
CLIP = 0.8
CLIP32 = float(np.float32(CLIP))                    # what a float kernel argument and torch's fp32 clamp_ make of 0.8


def _sgd64(p, g, buf, lr, momentum, dampening, weight_decay, nesterov):
    """torch.optim.SGD on one fp64 tensor; `g` is the (already clamped) gradient, `buf` None before the first momentum step."""
    if weight_decay != 0:
        g = g + weight_decay * p
    if momentum != 0:
        buf = g.clone() if buf is None else momentum * buf + (1 - dampening) * g
        g = g + momentum * buf if nesterov else buf
    return p - lr * g, buf


class _Twins(object):
    """The two oracles of one optimizer: torch.optim.SGD on CPU fp32 copies (o_c, pc) and the fp64 restatement (p64, b64).
    Schedulers act on o_c; the restatement reads its lr there at every step."""

    def __init__(self, values, groups, hyper):
        self.groups, self.hyper = groups, hyper
        self.pc = [v.detach().cpu().clone().requires_grad_(True) for v in values]
        self.o_c = torch.optim.SGD([dict(params=[self.pc[i] for i in idx], lr=lr) for idx, lr in groups], **hyper)
        self.p64 = [v.detach().cpu().double() for v in values]
        self.b64 = [None] * len(values)

    def step(self, grads, clip):
        """grads: CPU fp32 tensors or None.  Returns the clamped gradients."""
        clamped = [None if g is None else (g.clone().clamp_(-clip, clip) if clip else g.clone()) for g in grads]
        for gi, (idx, _) in enumerate(self.groups):
            lr = self.o_c.param_groups[gi]['lr']
            for i in idx:
                self.pc[i].grad = clamped[i]
                if clamped[i] is not None:
                    self.p64[i], self.b64[i] = _sgd64(self.p64[i], clamped[i].double(), self.b64[i], lr, **self.hyper)
        self.o_c.step()
        return clamped

    def cpu_bufs(self):
        return [self.o_c.state[p].get('momentum_buffer') if p in self.o_c.state else None for p in self.pc]


def _gate(got, cpu, ref, what):
    """The gate of the module docstring over parallel lists of tensors (entries whose reference is None are absent on all sides)."""
    keep = [i for i, r in enumerate(ref) if r is not None]
    assert all((got[i] is None) == (ref[i] is None) == (cpu[i] is None) for i in range(len(ref))), what + ': a tensor is missing or surplus'
    if not keep:
        return
    got = [got[i].detach().cpu().double().reshape(-1) for i in keep]
    cpu = [cpu[i].detach().double().reshape(-1) for i in keep]
    ref = [ref[i].reshape(-1) for i in keep]
    assert all(torch.isfinite(t).all() for t in got + cpu + ref), what + ': non-finite value'
    e_gpu = max((a - r).abs().max().item() for a, r in zip(got, ref))
    e_cpu = max((c - r).abs().max().item() for c, r in zip(cpu, ref))
    mag = max(t.abs().max().item() for t in got + cpu + ref)
    ulp = float(np.spacing(np.float32(mag)))
    msg = '%s: GPU max err vs fp64 %.3e, CPU fp32 torch max err vs fp64 %.3e, ulp(%.3g) %.3e' % (what, e_gpu, e_cpu, mag, ulp)
    print(msg)
    assert e_gpu <= 2.0 * e_cpu + ulp, msg


def _problem(dev, seed):
    """Nine device parameters with .grad, each a view inside a canary-filled buffer: SIZES and two 777s on 16-byte
    boundaries, ODD_SIZE one float past one."""
    g = _gen(seed)
    carved = dict(p=_Carved(SIZES + (777, 777), dev), g=_Carved(SIZES + (777, 777), dev), po=_Carved((ODD_SIZE,), dev, shift=1),
                  go=_Carved((ODD_SIZE,), dev))
    views = [(carved['p'].views[i], carved['g'].views[i]) for i in range(len(SIZES))] + [(carved['po'].views[0], carved['go'].views[0])] + \
        [(carved['p'].views[i], carved['g'].views[i]) for i in (len(SIZES), len(SIZES) + 1)]
    pd = []
    for vp, vg in views:
        vp.copy_(torch.randn(vp.numel(), generator=g)); vg.zero_()
        p = vp.requires_grad_(True); p.grad = vg
        pd.append(p)
    assert pd[6].numel() == ODD_SIZE and pd[6].data_ptr() % 16 == 4 and all(p.data_ptr() % 16 == 0 for i, p in enumerate(pd) if i != 6)
    return g, carved, pd


def _device_optimizer(pd, hyper):
    return torch.optim.SGD([dict(params=[pd[i] for i in idx], lr=lr) for idx, lr in GROUPS], **hyper)


def _run(pkg, dev, hyper, clip, seed=60, steps=3, scheduler=False):
    """`steps` fused steps against both oracles, every check of the issue after each.  Returns the final bits."""
    g, carved, pd = _problem(dev, seed)
    o_d = _device_optimizer(pd, hyper)
    tw = _Twins(pd, GROUPS, hyper)
    grad_views = [p.grad for p in pd]
    if scheduler:
        scheds = [torch.optim.lr_scheduler.MultiStepLR(o, milestones=[1, 2], gamma=0.3) for o in (o_d, tw.o_c)]
    for step in range(1, steps + 1):
        what = 'sgd %s clip %s step %d' % (hyper, clip, step)
        grads = [torch.randn(p.numel(), generator=g) * 2 for p in pd]
        if step <= 2:
            grads[SKIP_TWICE] = None
        if step == 2:
            grads[SKIP_ONCE] = None
        before = [_bits(p) for p in pd]
        for p, view, gr in zip(pd, grad_views, grads):
            p.grad = None if gr is None else view.copy_(gr)
        clamped = tw.step(grads, clip)
        pkg.optim.clip_sgd_step(o_d, clip)
        for name, c in carved.items():
            c.assert_gaps_intact('%s, buffer %s' % (what, name))
        _gate(pd, tw.pc, tw.p64, what + ' params')
        bufs = [o_d.state[p].get('momentum_buffer') if p in o_d.state else None for p in pd]
        _gate(bufs, tw.cpu_bufs(), tw.b64, what + ' momentum_buffer')
        if hyper['momentum'] == 0:
            assert all(b is None for b in bufs), what + ': momentum == 0 must leave no momentum_buffer'
        for i, (p, gr, cl) in enumerate(zip(pd, grads, clamped)):
            if gr is None:
                assert p.grad is None and torch.equal(_bits(p), before[i]), '%s: tensor %d has no gradient and moved' % (what, i)
            else:
                assert torch.equal(_bits(p.grad), _bits(cl)), '%s: .grad of tensor %d is not the clamped gradient' % (what, i)
                assert not clip or p.grad.abs().max().item() <= CLIP32
                assert not torch.equal(_bits(p), before[i]), '%s: tensor %d did not move' % (what, i)
        if scheduler:
            lrs = [gr['lr'] for gr in o_d.param_groups]
            with warnings.catch_warnings():
                warnings.filterwarnings('error', message='Detected call of')       # clip_sgd_step counts as the optimizer's step
                for s in scheds:
                    s.step()
            now = [gr['lr'] for gr in o_d.param_groups]
            assert now == [gr['lr'] for gr in tw.o_c.param_groups] and now == pytest.approx([(0.3 if step <= 2 else 1.0) * lr for lr in lrs], rel=1e-12)
    return o_d, tw, pd, [(_bits(p), _bits(p.grad), None if b is None else _bits(b)) for p, b in zip(pd, bufs)]


def _hyper(momentum, nesterov, weight_decay, dampening):
    return dict(momentum=momentum, nesterov=nesterov, weight_decay=weight_decay, dampening=dampening)


GRID = [(_hyper(m, n, wd, d), clip)
        for (m, n), wd, d, clip in itertools.product(((0, False), (0.9, False), (0.9, True)), (0, 1e-4), (0, 0.1), (None, CLIP))
        if not (n and d)]                             # torch.optim.SGD: nesterov requires zero dampening


def _grid_id(case):
    h, clip = case
    return 'm%g%s-wd%g-d%g-clip%s' % (h['momentum'], 'n' if h['nesterov'] else '', h['weight_decay'], h['dampening'], clip)


@pytest.mark.parametrize('case', GRID, ids=_grid_id)
def test_clip_sgd_grid(pkg, dev, case):
    """Three steps: the first-step branch, the recurrent one, and on step 3 both in one launch (tensor SKIP_TWICE meets its
    first gradient while the others are on their third; tensor SKIP_ONCE resumes from the buffer of step 1)."""
    hyper, clip = case
    assert len(GRID) == 20
    o_d, _, pd, _ = _run(pkg, dev, hyper, clip)
    if hyper['momentum'] == 0:
        assert all(len(o_d.state[p]) == 0 for p in pd if p in o_d.state)
        assert all(len(s) == 0 for s in o_d.state_dict()['state'].values())


def test_clip_sgd_is_reproducible(pkg, dev):
    hyper = _hyper(0.9, True, 1e-4, 0)
    a = _run(pkg, dev, hyper, CLIP)[3]
    b = _run(pkg, dev, hyper, CLIP)[3]
    for i, (x, y) in enumerate(zip(a, b)):
        assert all(torch.equal(s, t) for s, t in zip(x, y)), 'tensor %d differs between two identical runs' % i


def test_clip_sgd_follows_multisteplr(pkg, dev):
    """group['lr'] is read at every call: MultiStepLR scales both groups by 0.3 after step 1 and again after step 2."""
    _run(pkg, dev, _hyper(0.9, False, 1e-4, 0), CLIP, scheduler=True)


def test_clip_sgd_state_dict_round_trip(pkg, dev):
    """state_dict() of the device optimizer loads into a fresh CPU torch.optim.SGD: same buffers bit for bit, and one
    further step on each side from that common state still meets the gate."""
    hyper = _hyper(0.9, True, 1e-4, 0)
    o_d, _, pd, _ = _run(pkg, dev, hyper, CLIP, seed=61)
    tw = _Twins(pd, GROUPS, hyper)
    tw.o_c.load_state_dict(copy.deepcopy(o_d.state_dict()))
    for p, c in zip(pd, tw.pc):
        buf = tw.o_c.state[c]['momentum_buffer']
        assert buf.device.type == 'cpu' and torch.equal(_bits(buf), _bits(o_d.state[p]['momentum_buffer']))
    assert [{k: v for k, v in gr.items() if k != 'params'} for gr in tw.o_c.param_groups] == \
           [{k: v for k, v in gr.items() if k != 'params'} for gr in o_d.param_groups]
    tw.b64 = [b.double() for b in tw.cpu_bufs()]
    g = _gen(62)
    grads = [torch.randn(p.numel(), generator=g) * 2 for p in pd]
    for p, gr in zip(pd, grads):
        p.grad.copy_(gr)
    tw.step(grads, CLIP)
    pkg.optim.clip_sgd_step(o_d, CLIP)
    _gate(pd, tw.pc, tw.p64, 'step after the round trip, params')
    _gate([o_d.state[p]['momentum_buffer'] for p in pd], tw.cpu_bufs(), tw.b64, 'step after the round trip, momentum_buffer')


@pytest.mark.parametrize('shift', [0, 1])
def test_clip_sgd_momentum_buffer_guard_bands(pkg, dev, shift):
    """The helper allocates the momentum buffers itself, so here the kernel is launched on its plan directly with buffers
    carved out of a canary-filled allocation (`shift` floats past a 16-byte boundary: float4 body or scalar loop): first
    step (the canary inside [0, numel) is overwritten, never read) and recurrent step.  The bits are those of
    clip_sgd_step on ordinary tensors, whichever loop ran."""
    L = pkg._lib
    hyper = _hyper(0.9, True, 1e-4, 0)
    g = _gen(63)
    values = [torch.randn(n, generator=g) for n in SIZES]
    grads = [[torch.randn(n, generator=g) * 2 for n in SIZES] for _ in range(2)]
    # the helper on plain tensors
    plain = [v.to(dev).requires_grad_(True) for v in values]
    o_plain = torch.optim.SGD(plain, lr=5e-2, **hyper)
    for step in range(2):
        for p, gr in zip(plain, grads[step]):
            p.grad = gr.to(dev)
        pkg.optim.clip_sgd_step(o_plain, CLIP)
    # the same two launches with carved buffers
    cp, cg, cb = _Carved(SIZES, dev), _Carved(SIZES, dev), _Carved(SIZES, dev, shift=shift)
    params = []
    for vp, vg, v in zip(cp.views, cg.views, values):
        vp.copy_(v)
        p = vp.requires_grad_(True); p.grad = vg
        params.append(p)
    for step in range(2):
        for p, gr in zip(params, grads[step]):
            p.grad.copy_(gr)
        ptrs, sizes, blk_t, blk_c, nblk = pkg.optim._sgd_plan(params, cb.views, [step == 0] * len(params), dev)
        assert nblk == sum((n + 4095) // 4096 for n in SIZES)
        L.call('ssg_clamp_sgd_multi_f32', L.ptr(ptrs), L.ptr(sizes), L.ptr(blk_t), L.ptr(blk_c), nblk, CLIP, 5e-2, 0.9, 0.0, 1e-4, 1, L.stream_ptr())
        for c, name in ((cp, 'params'), (cg, 'grads'), (cb, 'momentum buffers')):
            c.assert_gaps_intact('step %d, %s' % (step + 1, name))
    for i, (p, q, b) in enumerate(zip(params, plain, cb.views)):
        assert torch.equal(_bits(p), _bits(q)) and torch.equal(_bits(p.grad), _bits(q.grad)), 'tensor %d' % i
        assert torch.equal(_bits(b), _bits(o_plain.state[q]['momentum_buffer'])), 'momentum buffer %d' % i


def test_unsupported_sgd_keeps_the_torch_path(pkg, dev, monkeypatch):
    """maximize=True: clip_sgd_step refuses, _step_optimizer clamps and steps it through torch as before."""
    T = pkg.train_seg_gan
    g = _gen(64)
    values = [torch.randn(n, generator=g) for n in (5, 4097)]
    grads = [torch.randn(v.numel(), generator=g) * 2 for v in values]
    kw = dict(lr=5e-2, momentum=0.9, maximize=True)
    pd = [v.to(dev).requires_grad_(True) for v in values]
    pc = [v.clone().requires_grad_(True) for v in values]
    for p, c, gr in zip(pd, pc, grads):
        p.grad = gr.to(dev); c.grad = gr.clamp(-CLIP, CLIP)
    o_d = torch.optim.SGD(pd, **kw); o_c = torch.optim.SGD(pc, **kw)
    with pytest.raises(NotImplementedError):
        pkg.optim.clip_sgd_step(o_d, CLIP)
    for p, v in zip(pd, values):
        assert torch.equal(p.detach().cpu(), v)
    monkeypatch.setattr(T, 'clip_sgd_step', lambda *a, **k: pytest.fail('clip_sgd_step called for an unsupported SGD'))
    T._step_optimizer(o_d, CLIP)
    o_c.step()
    for p, c in zip(pd, pc):
        assert torch.equal(p.grad.cpu(), c.grad)
        assert torch.allclose(p.detach().cpu(), c.detach(), rtol=0, atol=2.0 ** -22 * 4)
        assert torch.allclose(o_d.state[p]['momentum_buffer'].cpu(), o_c.state[c]['momentum_buffer'], rtol=0, atol=0)


# ============================================================================= trainer level
SGD_KW = dict(lr=1e-2, momentum=0.9, nesterov=True, weight_decay=1e-4)


class _Recorder(object):
    """Stands in for a trainer module's `clip_sgd_step`: snapshots the optimizer's parameters and gradients, runs the real
    step, snapshots the result."""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __call__(self, optimizer, grad_clip=None):
        params = [p for gr in optimizer.param_groups for p in gr['params']]
        before = [(p.detach().cpu().clone(), None if p.grad is None else p.grad.detach().cpu().clone()) for p in params]
        had = [p in optimizer.state and optimizer.state[p].get('momentum_buffer') is not None for p in params]
        self.real(optimizer, grad_clip)
        after = [p.detach().cpu().clone() for p in params]
        bufs = [optimizer.state[p]['momentum_buffer'].cpu().clone() if p in optimizer.state and 'momentum_buffer' in optimizer.state[p]
                else None for p in params]
        self.calls.append(dict(optimizer=optimizer, clip=grad_clip, before=before, had=had, after=after, bufs=bufs))


def _check_first_step(call, kw, what):
    """One recorded call on an optimizer without momentum buffers against both oracles."""
    assert not any(call['had'])
    hyper = dict(_hyper(0, False, 0, 0), **{k: v for k, v in kw.items() if k != 'lr'})
    values = [p for p, _ in call['before']]
    tw = _Twins(values, ((tuple(range(len(values))), kw['lr']),), hyper)
    tw.step([g for _, g in call['before']], call['clip'])
    assert sum(g is not None for _, g in call['before']) > len(values) // 2, what + ': most parameters should have a gradient'
    _gate(call['after'], tw.pc, tw.p64, what + ' params')
    _gate(call['bufs'], tw.cpu_bufs(), tw.b64, what + ' momentum_buffer')


def test_gan_step_with_sgd_runs_the_fused_step(pkg, dev, monkeypatch):
    """One stage-2 step, both nets on SGD: _step_optimizer hands each to clip_sgd_step with the reference's clip of 0.8, and
    what the G step and the D step did to the parameters is CPU torch's clamp_ + SGD.step() on the snapshots."""
    import torch.nn as nn
    from oracle import seg_gan_cpu as O
    T = pkg.train_seg_gan
    rec = _Recorder(T.clip_sgd_step)
    monkeypatch.setattr(T, 'clip_sgd_step', rec)
    monkeypatch.setattr(T, 'clip_adam_step', lambda *a, **k: pytest.fail('the Adam step ran'))
    torch.manual_seed(41)
    G = pkg.models_seg_gan.Generator(dict(arch='UNet_R_SS_v2', num_classes=3, input_channels=3, deep_supervision=False))
    D = pkg.models_seg_gan.Discriminator(3, 3, 64, 8, 1024)
    G.to(dev).train(); D.to(dev).train()
    og = torch.optim.SGD(G.parameters(), **SGD_KW); od = torch.optim.SGD(D.parameters(), **SGD_KW)
    inp, tgt = O.synthetic_batch(2, 64, 64)
    out = T.gan_step(inp.to(dev), tgt.to(dev), G, D, pkg.losses.BCEDiceLoss(), nn.BCEWithLogitsLoss(), nn.MSELoss(), og, od, 3)
    assert all(torch.isfinite(v).all() for v in out)
    assert [c['optimizer'] for c in rec.calls] == [og, od] and [c['clip'] for c in rec.calls] == [T.GRAD_CLIP, T.GRAD_CLIP] == [0.8, 0.8]
    for call, net, name in zip(rec.calls, (G, D), ('G', 'D')):
        _check_first_step(call, SGD_KW, 'gan_step %s' % name)
        for p, a in zip(net.parameters(), call['after']):                      # nothing moved them afterwards
            assert torch.equal(p.detach().cpu(), a)
        assert max(g.abs().max().item() for p in net.parameters() for g in [p.grad] if g is not None) <= CLIP32


def test_stage1_train_with_sgd_runs_the_fused_step(pkg, dev, monkeypatch):
    """One stage-1 iteration over a one-item loader at epoch 2, the optimizer and the cnn_optimizer both SGD: two fused
    steps without gradient clipping (stage 1 has none), the second on the first one's result."""
    M = pkg.train
    rec = _Recorder(M.clip_sgd_step)
    monkeypatch.setattr(M, 'clip_sgd_step', rec)
    monkeypatch.setattr(M, 'clip_adam_step', lambda *a, **k: pytest.fail('the Adam step ran'))
    torch.manual_seed(41)
    model = pkg.archs.UNet_R_SS_v2(3, 3, False).to(dev)
    opt = torch.optim.SGD(model.parameters(), **SGD_KW)
    cnn_kw = dict(lr=1e-3, momentum=0.5)
    cnn_opt = torch.optim.SGD(list(model.parameters())[:6], **cnn_kw)
    g = _gen(7)
    inp = torch.randn(2, 3, 64, 64, generator=g); tgt = (torch.rand(2, 3, 64, 64, generator=g) > 0.5).float()
    r = M.train(2, dict(clip=0.7, num_classes=3, deep_supervision=False), [(None, inp, tgt, None, None)], model,
                pkg.losses.BCEDiceLoss(), opt, cnn_opt)
    assert all(np.isfinite(v) for v in r.values())
    assert [c['optimizer'] for c in rec.calls] == [opt, cnn_opt] and [c['clip'] for c in rec.calls] == [None, None]
    _check_first_step(rec.calls[0], SGD_KW, 'stage 1 optimizer')
    _check_first_step(rec.calls[1], cnn_kw, 'stage 1 cnn_optimizer')
    for (b, _), a in zip(rec.calls[1]['before'], rec.calls[0]['after']):       # the second step starts from the first one's result
        assert torch.equal(b, a)
