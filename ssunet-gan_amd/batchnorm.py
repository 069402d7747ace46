"""Synchronized BatchNorm, MI355X-native (mirrors the surface of the reference's vendored
Synchronized-BatchNorm-PyTorch: scripts/batchnorm.py + comm.py + replicate.py; unwired there --
SURVEY.md 8a row A9).

The reference synchronises replicas of ONE process over Python threads and queue.Queue rendezvous
(comm.py:18-138), reducing [sum, ssum] to a master device and broadcasting [mean, inv_std] back
(batchnorm.py:92-113).  Here every GPU is its own process: the fp64 [sum, ssum] vector is all-reduced
over RCCL between the two kernel stages of the batch norm, every rank evaluates
`_compute_mean_std` (batchnorm.py:115-127: mean = sum/n, biased var, inv_std = clamp(var, eps)^-1/2,
running_var from the unbiased var) itself, and backward all-reduces [sum g, sum g*xhat] the same way.
"""
import functools

import torch.nn as nn

from . import dp, ops
from ._lib import ACT_NONE

__all__ = ['SynchronizedBatchNorm1d', 'SynchronizedBatchNorm2d', 'SynchronizedBatchNorm3d', 'convert_model',
           'patch_sync_batchnorm', 'DataParallelWithCallback', 'patch_replication_callback', 'freeze_batch_norm',
           'unfreeze_batch_norm']


class _SynchronizedBatchNorm(nn.modules.batchnorm._BatchNorm):
    def __init__(self, num_features, eps=1e-5, momentum=0.1, affine=True):
        super().__init__(num_features, eps=eps, momentum=momentum, affine=affine)

    def _group(self):
        g = getattr(self, '_ssg_sync_group', None)
        if g is None and dp.is_dist():
            import torch.distributed as dist
            g = dist.group.WORLD
        return g

    def forward(self, input):
        shape = input.shape
        x = input if input.dim() == 4 else input.reshape(shape[0], shape[1], -1, 1)
        group = self._group()
        # batchnorm.py:52-55: single device or eval -> F.batch_norm (torch formula); parallel+train -> sync formula
        y = ops.batch_norm_act(x, self, act=ACT_NONE, group=group if self.training else None,
                               var_mode=(1 if (group is not None and self.training) else 0))
        return y if input.dim() == 4 else y.reshape(shape)


class SynchronizedBatchNorm1d(_SynchronizedBatchNorm):
    pass


class SynchronizedBatchNorm2d(_SynchronizedBatchNorm):
    pass


class SynchronizedBatchNorm3d(_SynchronizedBatchNorm):
    pass


def convert_model(module):
    """batchnorm.py:313-361: swap every torch BatchNorm for its synchronized twin (weights shared)."""
    mod = module
    for src, dst in ((nn.BatchNorm1d, SynchronizedBatchNorm1d), (nn.BatchNorm2d, SynchronizedBatchNorm2d),
                     (nn.BatchNorm3d, SynchronizedBatchNorm3d)):
        if isinstance(module, src) and not isinstance(module, _SynchronizedBatchNorm):
            mod = dst(module.num_features, module.eps, module.momentum, module.affine)
            mod.running_mean, mod.running_var = module.running_mean, module.running_var
            mod.num_batches_tracked = module.num_batches_tracked
            if module.affine:
                mod.weight, mod.bias = module.weight, module.bias
    for name, child in module.named_children():
        mod.add_module(name, convert_model(child))
    return mod


def patch_sync_batchnorm(module, group=None):
    """In-place alternative to convert_model: keep the modules, mark them synchronized."""
    return dp.convert_sync_batchnorm(module, group)


def _frozen_train(self, mode=True):
    """nn.Module.train of a frozen batch norm: the children follow `mode`, the layer itself stays in eval mode."""
    nn.Module.train(self, mode)
    self.training = False
    return self


def freeze_batch_norm(module, freeze_affine=False):
    """Fine-tuning with frozen batch-norm statistics: every _BatchNorm under `module` goes to eval mode and STAYS there through
    later `module.train()` calls (both trainers call .train() every epoch).  Such a layer normalises with its running estimates,
    writes none of them (num_batches_tracked included), issues no sync-BN collective, and stays differentiable in its input and in
    gamma / beta.  `freeze_affine=True` also sets requires_grad_(False) on gamma / beta.  Returns the number of layers frozen."""
    n = 0
    for m in module.modules():
        if isinstance(m, nn.modules.batchnorm._BatchNorm):
            if '_ssg_frozen' not in m.__dict__:
                m.__dict__['_ssg_frozen'] = tuple(p.requires_grad for p in (m.weight, m.bias) if p is not None)
                # a partial of a module-level function: deepcopy and pickle (torch.save(model), spawn) carry it along
                m.train = functools.partial(_frozen_train, m)
            m.training = False
            if freeze_affine:
                for p in (m.weight, m.bias):
                    if p is not None:
                        p.requires_grad_(False)
            n += 1
    return n


def unfreeze_batch_norm(module):
    """Undo freeze_batch_norm: the layers follow .train() / .eval() again (each takes the mode of its parent now) and gamma / beta
    get back the requires_grad they had.  Returns the number of layers released."""
    n = 0
    if isinstance(module, nn.modules.batchnorm._BatchNorm) and '_ssg_frozen' in module.__dict__:
        n += _release(module, module.training)              # no parent to follow: it keeps its mode until the next .train()
    for parent in module.modules():
        for m in parent.children():
            if isinstance(m, nn.modules.batchnorm._BatchNorm) and '_ssg_frozen' in m.__dict__:
                n += _release(m, parent.training)
    return n


def _release(m, mode):
    was = m.__dict__.pop('_ssg_frozen')
    m.__dict__.pop('train', None)
    for p, rg in zip([p for p in (m.weight, m.bias) if p is not None], was):
        p.requires_grad_(rg)
    m.training = mode
    return 1


class DataParallelWithCallback(nn.Module):
    """replicate.py:50-67 wrapped nn.DataParallel so replicas could rendezvous.  With one process per
    GPU there is nothing to replicate: this keeps the name and simply forwards to the wrapped module."""

    def __init__(self, module, device_ids=None, output_device=None, dim=0):
        super().__init__()
        self.module = module

    def forward(self, *a, **k):
        return self.module(*a, **k)


def patch_replication_callback(data_parallel):
    return data_parallel
