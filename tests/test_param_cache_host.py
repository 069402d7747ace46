"""The stamps of the parameter-derived caches, driven with CPU tensors: the stamp logic is pure Python and torch.

For each of ops._stamped_cache (the `_ssg_pack*` caches), blocks._spade_cat (`_ssg_gb_cat`) and archs.BasicBlock._folded /
._fold_consts (`_fold_cache`, `_fold_consts_cache`) this pins which events start a new entry -- an in-place op, copy_,
load_state_dict, `p.data = t`, bump_weight_epoch and, for the folds, a move of the running-statistics epoch -- and which do not:
a write through `.data` without a bump, the documented limitation.  The device half (the same events against the kernels' output)
is tests/test_param_contract_gpu.py."""
import copy

import pytest
import torch
import torch.nn as nn


@pytest.fixture
def ops(pkg):
    return pkg.ops


def _param(*shape):
    return nn.Parameter(torch.randn(*shape, generator=torch.Generator().manual_seed(sum(shape))))


def _inplace(p, keep):
    with torch.no_grad():
        p.mul_(1.5)


def _copy(p, keep):
    with torch.no_grad():
        p.copy_(torch.full_like(p, 0.25))


def _set_data(p, keep):
    keep.append(p.data)                         # the old storage stays alive: its address cannot come back for the new one
    p.data = torch.full_like(p, 0.5)


def _bump(ops):
    return lambda p, keep: ops.bump_weight_epoch()


def _data_write(p, keep):
    p.data.mul_(3.0)                            # invisible to p._version: stays stale until somebody bumps the epoch


TENSOR_EVENTS = [('inplace', _inplace), ('copy_', _copy), ('data=', _set_data)]


# ----------------------------------------------------------------------------------------------------------- ops._stamped_cache
@pytest.mark.parametrize('event', [e[0] for e in TENSOR_EVENTS] + ['bump'])
def test_stamped_cache_starts_over(ops, event):
    fn = dict(TENSOR_EVENTS, bump=_bump(ops))[event]
    p, keep = _param(4, 3, 3, 3), []
    c0 = ops._stamped_cache(p, '_ssg_pack')
    c0['key'] = 'packed'
    assert ops._stamped_cache(p, '_ssg_pack') is c0 and '_ssg_pack' in p.__dict__
    fn(p, keep)
    c1 = ops._stamped_cache(p, '_ssg_pack')
    assert c1 is not c0 and c1 == {}, event
    assert ops._stamped_cache(p, '_ssg_pack') is c1


def test_stamped_cache_load_state_dict(ops):
    m = nn.Conv2d(3, 4, 3)
    c0 = ops._stamped_cache(m.weight, '_ssg_pack'); c0['key'] = 1
    m.load_state_dict({k: v + 1 for k, v in m.state_dict().items()})
    assert ops._stamped_cache(m.weight, '_ssg_pack') == {}


def test_stamped_cache_data_write_is_seen_only_after_a_bump(ops):
    p = _param(4, 3, 3, 3)
    c0 = ops._stamped_cache(p, '_ssg_pack'); c0['key'] = 1
    _data_write(p, [])
    assert ops._stamped_cache(p, '_ssg_pack') is c0             # the documented limitation: raw writers must bump
    ops.bump_weight_epoch()
    assert ops._stamped_cache(p, '_ssg_pack') == {}


def test_stamped_cache_ignores_the_statistics_epoch_and_other_names(ops):
    p = _param(4, 3, 3, 3)
    c0 = ops._stamped_cache(p, '_ssg_pack'); c0['key'] = 1
    x1 = ops._stamped_cache(p, '_ssg_pack_bf16x1'); x1['key'] = 2
    ops._STATS_EPOCH[0] += 1                                    # running statistics are no source of a weight pack
    assert ops._stamped_cache(p, '_ssg_pack') is c0 and ops._stamped_cache(p, '_ssg_pack_bf16x1') is x1 and x1 is not c0


def test_one_stamp_function(ops):
    """Every cache stamps through ops._stamp: sources' (address, version), the optimizer epoch, optionally the statistics epoch."""
    a, b = _param(3), _param(5)
    s = ops._stamp((a, b))
    assert s == ((a.data_ptr(), a._version), (b.data_ptr(), b._version), ops._WEIGHT_EPOCH[0])
    assert ops._stamp((a,), stats=True) == ((a.data_ptr(), a._version), ops._WEIGHT_EPOCH[0], ops._STATS_EPOCH[0])


def test_deepcopy_of_a_parameter_carries_no_cache(ops):
    p = _param(4, 3, 3, 3)
    ops._stamped_cache(p, '_ssg_pack')['key'] = torch.zeros(3)
    ops._stamped_cache(p, '_ssg_pack_bf16')['key'] = torch.zeros(3)
    q = copy.deepcopy(p)
    assert [k for k in q.__dict__ if k.startswith('_ssg_')] == []
    m = nn.Conv2d(3, 4, 3)
    ops._stamped_cache(m.weight, '_ssg_pack')['key'] = torch.zeros(3)
    m2 = copy.deepcopy(m)
    assert [k for k in m2.weight.__dict__ if k.startswith('_ssg_')] == []


# ----------------------------------------------------------------------------------------------------------- blocks._spade_cat
def _spade_sources():
    return _param(8, 4, 3, 3), _param(8), _param(8, 4, 3, 3) , _param(8)


@pytest.mark.parametrize('which', range(4))
@pytest.mark.parametrize('event', [e[0] for e in TENSOR_EVENTS] + ['bump'])
def test_spade_cat_follows_every_source(pkg, ops, event, which):
    fn = dict(TENSOR_EVENTS, bump=_bump(ops))[event]
    srcs, keep = _spade_sources(), []
    w0, b0 = pkg.blocks._spade_cat(*srcs)
    assert pkg.blocks._spade_cat(*srcs)[0] is w0
    fn(srcs[which], keep)
    w1, b1 = pkg.blocks._spade_cat(*srcs)
    assert w1 is not w0 and b1 is not b0, (event, which)
    assert torch.equal(w1, torch.cat([srcs[0], srcs[2]]).detach()) and torch.equal(b1, torch.cat([srcs[1], srcs[3]]).detach())
    assert not w1.requires_grad and w1.is_contiguous()


def test_spade_cat_data_write_is_seen_only_after_a_bump(pkg, ops):
    srcs = _spade_sources()
    w0, _ = pkg.blocks._spade_cat(*srcs)
    _data_write(srcs[2], [])
    assert pkg.blocks._spade_cat(*srcs)[0] is w0
    ops.bump_weight_epoch()
    w1, _ = pkg.blocks._spade_cat(*srcs)
    assert w1 is not w0 and torch.equal(w1[8:], srcs[2].detach())


# ----------------------------------------------------------------------------------------------------------- BasicBlock folds
def _block(pkg):
    torch.manual_seed(3)
    b = pkg.archs.BasicBlock(4, 8).eval()
    with torch.no_grad():
        for bn in (b.bn1, b.bn2):
            bn.weight.uniform_(0.5, 1.5); bn.bias.normal_(); bn.running_mean.normal_(); bn.running_var.uniform_(0.5, 2.0)
    return b


def _fold_ref(b):
    out = []
    for conv, bn in ((b.conv1, b.bn1), (b.conv2, b.bn2)):
        s = bn.weight.detach() * torch.rsqrt(bn.running_var + bn.eps)
        out += [conv.weight.detach() * s.view(-1, 1, 1, 1), bn.bias.detach() - bn.running_mean * s]
    return out


FOLD_SOURCES = ['conv1.weight', 'conv2.weight', 'bn1.weight', 'bn1.bias', 'bn1.running_mean', 'bn1.running_var',
                'bn2.weight', 'bn2.bias', 'bn2.running_mean', 'bn2.running_var']
CONST_SOURCES = [s for s in FOLD_SOURCES if not s.startswith('conv') and not s.endswith('bias')]


def _get(b, path):
    mod, name = path.split('.')
    return getattr(getattr(b, mod), name)


@pytest.mark.parametrize('src', FOLD_SOURCES)
@pytest.mark.parametrize('event', [e[0] for e in TENSOR_EVENTS])
def test_folds_follow_every_source(pkg, event, src):
    fn = dict(TENSOR_EVENTS)[event]
    b, keep = _block(pkg), []
    f0, k0 = b._folded(), b._fold_consts()
    assert b._folded() is f0 and b._fold_consts() is k0
    fn(_get(b, src), keep)
    f1 = b._folded()
    assert f1 is not f0, (event, src)
    for got, ref in zip(f1, _fold_ref(b)):
        torch.testing.assert_close(got, ref, rtol=0, atol=0)
    if src in CONST_SOURCES:
        k1 = b._fold_consts()
        assert k1 is not k0, (event, src)
        for (s, mean, invstd), bn in zip(k1, (b.bn1, b.bn2)):
            assert torch.equal(invstd, torch.rsqrt(bn.running_var + bn.eps)) and torch.equal(mean, bn.running_mean)
            assert torch.equal(s, bn.weight.detach() * invstd)


def test_folds_follow_the_epochs_and_load_state_dict(pkg, ops):
    b = _block(pkg)
    for event in ('bump', 'stats', 'load'):
        f0, k0 = b._folded(), b._fold_consts()
        if event == 'bump':
            ops.bump_weight_epoch()
        elif event == 'stats':
            ops._STATS_EPOCH[0] += 1            # what a training-mode batch norm does after its raw-pointer write of the statistics
        else:
            b.load_state_dict({k: (v * 1.25 if v.is_floating_point() else v) for k, v in b.state_dict().items()})
        assert b._folded() is not f0 and b._fold_consts() is not k0, event
    for got, ref in zip(b._folded(), _fold_ref(b)):
        assert torch.equal(got, ref)


def test_folds_data_write_is_seen_only_after_a_bump(pkg, ops):
    b = _block(pkg)
    f0, k0 = b._folded(), b._fold_consts()
    _data_write(b.bn1.weight, [])
    assert b._folded() is f0 and b._fold_consts() is k0
    ops.bump_weight_epoch()
    assert b._folded() is not f0 and b._fold_consts() is not k0
    assert torch.equal(b._folded()[0], _fold_ref(b)[0])


def test_deepcopied_block_refolds_on_its_own(pkg):
    b = _block(pkg)
    f0, k0 = b._folded(), b._fold_consts()
    b2 = copy.deepcopy(b)
    f2 = b2._folded()
    assert all(a is not c and a.data_ptr() != c.data_ptr() and torch.equal(a, c) for a, c in zip(f2, f0))
    with torch.no_grad():
        b2.conv1.weight.mul_(2.0); b2.bn2.running_var.fill_(4.0)
    for got, ref in zip(b2._folded(), _fold_ref(b2)):
        assert torch.equal(got, ref)
    assert torch.equal(b2._fold_consts()[1][2], torch.rsqrt(b2.bn2.running_var + b2.bn2.eps))
    assert b._folded() is f0 and b._fold_consts() is k0         # the original's folds are its own
    for got, ref in zip(f0, _fold_ref(b)):
        assert torch.equal(got, ref)
