"""The NHWC memory contract (head of ops.py) looked at in memory, not through the logical [N, C, H, W] view:

* every op runs under tests/layout_probe.py's guarded allocator: each tensor the library allocates for itself must come back
  completely written, with zero pad lanes [C, pad4(C)) and with untouched guard bands in front of and behind it;
* every op that takes an NHWC input with C % 4 == 0 runs again with that input as a channel slice of a wider canary-filled
  buffer (pixel stride ld > C): same bits as the compact run where the same kernels ran, no NaN, neighbours untouched -- or a
  pinned exception where the op has no strided form;
* _conv_fwd_impl(..., out=) writes into a channel slice of a wider buffer for every conv family.

Values are compared with an fp64 CPU reference of the same op at the tolerance that op already has in tests/test_ops_gpu.py
(quoted at each use).  Ops without an op-level test of their own borrow the formula of the nearest one, named where it is used:
channel_scale's gate gradient that of dwconv2d's bias gradient (a sum over the pixels), conv2d_sn those of conv2d, seg_loss the
sum of its two scalar bounds, se_gate the bound of tests/test_round3_gpu.py; max_pool2x2_skip's backward, one fp32 add, is bounded
by one ulp."""
import math
import re
import types

import pytest
import torch
import torch.nn.functional as F

import layout_probe as lp
from test_ops_gpu import CONV_CASES, KERNEL_CASES, _close, _k32_label, _split_label

pytestmark = pytest.mark.gpu

# names of ops.__all__ (+ the four public ops it leaves out) that neither take nor produce an NHWC tensor
EXEMPT = {
    'bump_weight_epoch': 'bumps a host-side counter; no tensor',
    'spectral_norm_weight': 'OIHW weight, u, v vectors in; OIHW weight and a scalar out',
    'bce_with_logits_const': '[N, 1] logits in, a scalar out (its gradient buffer is not an NHWC tensor)',
    'new_nhwc': 'the allocator itself: replaced by the guarded one in every test here',
}
EXTRA_PUBLIC = ('add', 'concat_channels', 'pixel_gate', 'se_gate')
ODD_CHANNELS = (1, 2, 3, 5, 6, 7, 66)           # 3, 2, 1 pad lanes twice over, and one group + a ragged quad


@pytest.fixture
def guard(pkg, dev, monkeypatch):
    alloc = lp.GuardedAllocator().install(monkeypatch, pkg)
    yield alloc
    alloc.check()                               # non-empty record + whatever was allocated after the test's last check


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _no_nan(t, what):
    assert not torch.isnan(t).any(), '%s holds a NaN' % what


# ----------------------------------------------------------------------------------------------------------- generic op runner
def _case(xs, dev_fn, ref_fn, tol_f, tol_b, ps=(), fwd_only=False):
    """xs: CPU fp32 NHWC-able inputs (the ones a channel slice can replace); ps: other differentiable operands (weights);
    dev_fn(pkg, xs, ps) / ref_fn(xs, ps) -> tensor or tuple of tensors; tol_f = (rtol, atol) of the outputs; tol_b = one
    (rtol, atol) per entry of xs + ps (None: no gradient expected)."""
    return dict(xs=list(xs), ps=list(ps), dev=dev_fn, ref=ref_fn, tol_f=tol_f, tol_b=list(tol_b), fwd_only=fwd_only)


def _tup(y):
    return tuple(y) if isinstance(y, (tuple, list)) else (y,)


def _reference(case, seed=99):
    xs = [x.double().requires_grad_(True) for x in case['xs']]
    ps = [p.double().requires_grad_(True) for p in case['ps']]
    ys = _tup(case['ref'](xs, ps))
    g = _gen(seed)
    dys = [torch.randn(y.shape, generator=g) for y in ys]
    if not case['fwd_only']:
        torch.autograd.backward(list(ys), [d.double() for d in dys])
    return [y.detach() for y in ys], dys, [t.grad for t in xs + ps]


def _compact(pkg, dev):
    return lambda i, x: pkg.ops.to_nhwc(x.to(dev)) if x.dim() == 4 else x.to(dev)


def _execute(pkg, dev, alloc, case, dys, place, dy_place=None):
    """One forward + backward on the device under the guards; returns (outputs, gradients, PROFILE labels, placed inputs)."""
    ops = pkg.ops
    xs = [place(i, x) for i, x in enumerate(case['xs'])]
    if not case['fwd_only']:
        xs = [x.requires_grad_(True) for x in xs]
    ps = [p.to(dev).requires_grad_(not case['fwd_only']) for p in case['ps']]
    ops.PROFILE = []
    try:
        ys = _tup(case['dev'](pkg, xs, ps))
        alloc.check()
        if not case['fwd_only']:
            gs = [(dy_place(d) if (dy_place is not None and d.dim() == 4 and d.shape[1] % 4 == 0) else d.to(dev)) for d in dys]
            torch.autograd.backward(list(ys), gs)
            alloc.check()
        labels = [r[0] for r in ops.PROFILE]
    finally:
        ops.PROFILE = None
    return [y.detach() for y in ys], [t.grad for t in xs + ps], labels, xs


def _compare(case, got_y, got_g, ref_y, ref_g, what):
    for k, (a, b) in enumerate(zip(got_y, ref_y)):
        _no_nan(a, '%s output %d' % (what, k))
        assert tuple(a.shape) == tuple(b.shape), (what, a.shape, b.shape)
        _close(a, b, case['tol_f'][0], case['tol_f'][1], '%s output %d' % (what, k))
    if case['fwd_only']:
        return
    for k, (a, b, tol) in enumerate(zip(got_g, ref_g, case['tol_b'])):
        if tol is None or b is None:
            continue
        assert a is not None, '%s: no gradient for operand %d' % (what, k)
        _no_nan(a, '%s gradient %d' % (what, k))
        _close(a.reshape(b.shape), b, tol[0], tol[1], '%s gradient %d' % (what, k))


def _placements(c):
    """(c0, ld): the slice in the first lanes of a wider buffer (ld = C + 4, ld = 2C) and in the middle of one
    (c0 = 4 of C + 8, the upper half of 2C)."""
    return [(0, c + 4), (0, 2 * c), (4, c + 8), (c, 2 * c)]


def _slice_runs(pkg, dev, alloc, case, what, expect_raise=None, switch=None):
    """The compact run against fp64, then the same op with its NHWC inputs (C % 4 == 0) and the incoming gradient as channel
    slices: all together at each placement, each alone at the mid-buffer one.  Equal PROFILE labels -> bit-identical results;
    a different kernel for the wide stride must be pinned in `switch` and is compared with fp64 at the op's tolerance."""
    ops = pkg.ops
    ref_y, dys, ref_g = _reference(case)
    y0, g0, l0, _ = _execute(pkg, dev, alloc, case, dys, _compact(pkg, dev))
    _compare(case, y0, g0, ref_y, ref_g, what + ' compact')
    able = [i for i, x in enumerate(case['xs']) if x.dim() == 4 and x.shape[1] % 4 == 0]
    assert able or expect_raise is not None, what + ': no input a channel slice can replace'
    runs = [('all', k, set(able), True) for k in range(4)] + [('only %d' % i, 2, {i}, False) for i in able] + [('only dy', 2, set(), True)]
    pairs = set()
    for tag, k, which, slice_dy in runs:
        made = []

        def place(i, x):
            if i not in which:
                return _compact(pkg, dev)(i, x)
            c0, ld = _placements(x.shape[1])[k]
            v = lp.poisoned_slice(x, ld, c0, dev)
            assert ops.nhwc_ld(v) == ld and ops.to_nhwc(v) is v        # the kernels, not a hidden copy, see the wide stride
            made.append(v)
            return v

        def dy_place(d):
            c0, ld = _placements(d.shape[1])[k]
            v = lp.poisoned_slice(d, ld, c0, dev)
            made.append(v)
            return v
        if expect_raise is not None and which and (expect_raise[1] is None or which & expect_raise[1]):
            with pytest.raises(expect_raise[0]):
                _execute(pkg, dev, alloc, case, dys, place, dy_place if slice_dy else None)
            for v in made:
                lp.check_slice(v)
            continue
        y1, g1, l1, _ = _execute(pkg, dev, alloc, case, dys, place, dy_place if (slice_dy and not case['fwd_only']) else None)
        name = '%s slices %s @%d' % (what, tag, k)
        for v in made:
            lp.check_slice(v)
        if l1 == l0:
            for a, b in zip(y1 + [g for g in g1 if g is not None], y0 + [g for g in g0 if g is not None]):
                _no_nan(a, name)
                assert torch.equal(a, b), '%s: differs from the compact run by %.3e' % (name, (a - b).abs().max().item())
        else:
            pairs.add((tuple(l0), tuple(l1)))
            assert switch is not None and (tuple(l0), tuple(l1)) in switch, \
                '%s: the wide stride changed the kernels %s -> %s (not a pinned switch)' % (name, l0, l1)
            _compare(case, y1, g1, ref_y, ref_g, name)
    return pairs


# ----------------------------------------------------------------------------------------------------------- the op table
# tolerances, by reference to tests/test_ops_gpu.py:
EW = (1e-6, 1e-6)               # test_pixel_gate: element-wise forward and dx; test_spade_modulate; test_adaptive_avgpool_flat
EWG = (1e-5, 1e-5)              # test_pixel_gate: dpsi (a gradient through the sigmoid's derivative)
EXACT = (0, 0)                  # test_pool_unpool


def _psum(n, h, w):             # test_dwconv2d, bias gradient: a channel sum over the pixels
    return (2e-5, 1e-5 * math.sqrt(n * h * w))


def _unary_case(name, c):
    x = torch.randn(2, c, 5, 7, generator=_gen(c))
    ref = {'swish': lambda t: t * torch.sigmoid(t), 'sigmoid': torch.sigmoid, 'gaussian': lambda t: torch.exp(-t * t)}[name]
    return _case([x], lambda pkg, xs, ps: getattr(pkg.ops, name)(xs[0]), lambda xs, ps: ref(xs[0]), EW, [EWG])


def _mul_case(c):
    g = _gen(10 + c)
    a = torch.randn(2, c, 5, 7, generator=g); b = torch.randn(2, c, 5, 7, generator=g)
    return _case([a, b], lambda pkg, xs, ps: pkg.ops.mul(xs[0], xs[1]), lambda xs, ps: xs[0] * xs[1], EW, [EW, EW])


def _add_case(c):
    g = _gen(20 + c)
    a = torch.randn(2, c, 5, 7, generator=g); b = torch.randn(2, c, 5, 7, generator=g)
    return _case([a, b], lambda pkg, xs, ps: pkg.ops.add(xs[0], xs[1]), lambda xs, ps: xs[0] + xs[1], EW, [EW, EW])


def _pixel_gate_case(c):
    g = _gen(30 + c)
    x = torch.randn(2, c, 9, 11, generator=g); p = torch.randn(2, 1, 9, 11, generator=g)
    return _case([x, p], lambda pkg, xs, ps: pkg.ops.pixel_gate(xs[0], xs[1]), lambda xs, ps: xs[0] * torch.sigmoid(xs[1]), EW, [EW, EWG])


def _channel_scale_case(c):
    g = _gen(40 + c)
    x = torch.randn(3, c, 5, 7, generator=g); s = torch.randn(3, c, 1, 1, generator=g)
    return _case([x, s], lambda pkg, xs, ps: pkg.ops.channel_scale(xs[0], xs[1]), lambda xs, ps: xs[0] * xs[1], EW, [EW, _psum(1, 5, 7)])


def _global_avgpool_case(c):
    x = torch.randn(3, c, 5, 7, generator=_gen(50 + c))
    return _case([x], lambda pkg, xs, ps: pkg.ops.global_avgpool(xs[0]), lambda xs, ps: F.adaptive_avg_pool2d(xs[0], 1), EW, [EW])


def _pool_case(skip):
    x = torch.randn(2, 8, 12, 16, generator=_gen(6))
    x[0, 0, 0, 0] = x[0, 0, 0, 1] = 5.0

    def dev_fn(pkg, xs, ps):
        if skip:
            y, _, xk = pkg.ops.max_pool2x2_skip(xs[0])
            return y, xk
        return pkg.ops.max_pool2x2(xs[0])[0]

    def ref_fn(xs, ps):
        y = F.max_pool2d(xs[0], 2, 2)
        return (y, xs[0] * 1.0) if skip else y
    # the skip form adds two fp32 gradients in its backward pass: one rounding of the sum, at most half an ulp (2^-24 relative),
    # bounded here by a whole one; the plain pool stays exact (test_pool_unpool)
    return _case([x], dev_fn, ref_fn, EXACT, [(2.0 ** -23, 0) if skip else EXACT])


def _unpool_case():
    g = _gen(7)
    src = torch.randn(2, 8, 12, 16, generator=g); z = torch.randn(2, 8, 6, 8, generator=g)
    _, ir = F.max_pool2d(src, 2, 2, return_indices=True)

    def dev_fn(pkg, xs, ps):
        _, idx = pkg.ops.max_pool2x2(src.to(xs[0].device))
        return pkg.ops.max_unpool2x2(xs[0], idx)
    return _case([z], dev_fn, lambda xs, ps: F.max_unpool2d(xs[0], ir, 2, 2), EXACT, [EXACT])


def _upsample_case(mode, shape):
    x = torch.randn(shape, generator=_gen(7))
    kw = dict(align_corners=True) if mode == 'bilinear' else {}
    grow = max(1.0, 2 * max(shape[2], shape[3]) / 16.0)          # test_upsample: the bound against the CPU grows with the image
    return _case([x], lambda pkg, xs, ps: getattr(pkg.ops, 'upsample2x_' + mode)(xs[0]),
                 lambda xs, ps: F.interpolate(xs[0], scale_factor=2, mode=mode, **kw), (1e-6 * grow, 1e-6 * grow), [(1e-5 * grow, 2e-6 * grow)])


def _modulate_case(c):
    g = _gen(10)
    x = torch.randn(2, c, 6, 6, generator=g); gb = torch.randn(2, 2 * c, 6, 6, generator=g)
    return _case([x, gb], lambda pkg, xs, ps: pkg.ops.spade_modulate(xs[0], xs[1]),
                 lambda xs, ps: xs[0] * (1 + xs[1][:, :c]) + xs[1][:, c:], EW, [EW, EW])


def _dwconv_case(n, c, h, w, k, stride, pad):
    g = _gen(c * 100 + k)
    x = torch.randn(n, c, h, w, generator=g); wt = torch.randn(c, 1, k, k, generator=g) / k; b = torch.randn(c, generator=g)
    # test_dwconv2d
    return _case([x], lambda pkg, xs, ps: pkg.ops.dwconv2d(xs[0], ps[0], ps[1], stride, pad),
                 lambda xs, ps: F.conv2d(xs[0], ps[0], ps[1], stride, pad, groups=c), (1e-5, 1e-5),
                 [(1e-5, 1e-5), (2e-5, 2e-5 * math.sqrt(n * h * w)), (2e-5, 1e-5 * math.sqrt(n * h * w))], ps=[wt, b])


def _bn_holder(w, b, rm, rv, training):
    return types.SimpleNamespace(training=training, track_running_stats=True, momentum=0.1, eps=1e-5, weight=w, bias=b,
                                 running_mean=rm, running_var=rv, num_batches_tracked=torch.zeros((), dtype=torch.long, device=w.device))


def _bn_case(shape, act, res, training=True):
    g = _gen(5)
    n, c, h, w = shape
    x = torch.randn(shape, generator=g) * 2 + 0.5
    wt = torch.rand(c, generator=g) + 0.5; b = torch.randn(c, generator=g)
    rm = torch.randn(c, generator=g); rv = torch.rand(c, generator=g) + 0.5
    fn = {'relu': F.relu, 'lrelu': lambda t: F.leaky_relu(t, 0.2), 'none': lambda t: t}[act]

    def dev_fn(pkg, xs, ps):
        code = {'relu': pkg._lib.ACT_RELU, 'lrelu': pkg._lib.ACT_LRELU, 'none': pkg._lib.ACT_NONE}[act]
        d = xs[0].device
        bn = _bn_holder(ps[0], ps[1], rm.to(d), rv.to(d), training)
        return pkg.ops.batch_norm_act(xs[0], bn, res=xs[1] if res else None, act=code, slope=0.2)

    def ref_fn(xs, ps):
        y = F.batch_norm(xs[0], rm.double(), rv.double(), ps[0], ps[1], training, 0.1, 1e-5)
        return fn(y + xs[1] if res else y)
    xs = [x] + ([torch.randn(shape, generator=g)] if res else [])
    # test_batch_norm_act: fwd, dx, dres, dweight, dbias
    return _case(xs, dev_fn, ref_fn, (1e-5, 1e-5), [(1e-4, 2e-5)] + ([(1e-6, 1e-6)] if res else []) + [(1e-4, 1e-4), (1e-4, 1e-4)],
                 ps=[wt, b], fwd_only=not training)


def _avgpool_flat_case(c, hw):
    x = torch.randn(2, c, *hw, generator=_gen(8))
    return _case([x], lambda pkg, xs, ps: pkg.ops.adaptive_avgpool_flat(xs[0], 6),
                 lambda xs, ps: F.adaptive_avg_pool2d(xs[0], (6, 6)).reshape(2, -1), EW, [EW])


def _seg_loss_case(c):
    from oracle import seg_gan_cpu as O
    g = _gen(11)
    x = torch.randn(3, c, 20, 24, generator=g) * 3
    t = (torch.rand(3, c, 20, 24, generator=g) > 0.5).float()

    def dev_fn(pkg, xs, ps):
        res = pkg.ops.seg_loss(xs[0], xs[1].detach(), min(1, c - 1))
        return res[0] + 0.3 * res[1]
    # test_seg_loss_vs_oracle: |loss| < 1e-5 on each scalar, gradient (1e-4, 1e-8)
    return _case([x, t], dev_fn, lambda xs, ps: O.bce_dice_loss(xs[0], xs[1].detach()) + 0.3 * F.mse_loss(xs[0], xs[1].detach()),
                 (0, 1.3e-5), [(1e-4, 1e-8), None])


def _concat_case():
    g = _gen(12)
    xs = [torch.randn(2, c, 5, 7, generator=g) for c in (4, 8, 12)]
    return _case(xs, lambda pkg, xs, ps: pkg.ops.concat_channels(*xs), lambda xs, ps: torch.cat(xs, 1), EXACT, [EXACT] * 3)


def _conv_sn_case():
    g = _gen(13)
    x = torch.randn(2, 16, 16, 16, generator=g); wt = torch.randn(32, 16, 3, 3, generator=g) / 12; b = torch.randn(32, generator=g)
    u = F.normalize(torch.randn(32, generator=g), dim=0); v = F.normalize(torch.randn(144, generator=g), dim=0)

    def dev_fn(pkg, xs, ps):
        d = xs[0].device
        return pkg.ops.conv2d_sn(xs[0], ps[0], u.to(d), v.to(d), ps[1], 1, 1, act=pkg._lib.ACT_LRELU, slope=0.2)

    def ref_fn(xs, ps):
        wm = ps[0].reshape(32, -1)
        with torch.no_grad():                                   # spectral_norm.py:73-88: one power iteration, u and v are constants
            v1 = F.normalize(wm.t() @ u.double(), dim=0, eps=1e-12); u1 = F.normalize(wm @ v1, dim=0, eps=1e-12)
        sigma = torch.dot(u1, wm @ v1)
        return F.leaky_relu(F.conv2d(xs[0], ps[0] / sigma, ps[1], 1, 1), 0.2)
    # test_conv2d_fwd_bwd's formulas: K = 144 forward, Cout * k * k for dx, pixels for dw
    return _case([x], dev_fn, ref_fn, (1e-5, 2e-6 * 12), [(1e-5, 2e-6 * math.sqrt(32 * 9)), (2e-5, 2e-6 * math.sqrt(2 * 256)), (2e-5, 1e-5)], ps=[wt, b])


def _op_table():
    t = []
    for c in ODD_CHANNELS + (8,):
        for name in ('swish', 'sigmoid', 'gaussian'):
            t.append(('%s-c%d' % (name, c), lambda name=name, c=c: _unary_case(name, c)))
        t.append(('mul-c%d' % c, lambda c=c: _mul_case(c)))
        t.append(('add-c%d' % c, lambda c=c: _add_case(c)))
        t.append(('pixel_gate-c%d' % c, lambda c=c: _pixel_gate_case(c)))
        t.append(('adaptive_avgpool_flat-c%d' % c, lambda c=c: _avgpool_flat_case(c, (7, 9))))
        t.append(('batch_norm_act-train-c%d' % c, lambda c=c: _bn_case((2, c, 8, 9), 'relu', c % 2 == 1)))
        t.append(('batch_norm_act-eval-c%d' % c, lambda c=c: _bn_case((2, c, 8, 9), 'lrelu', c % 2 == 0, training=False)))
    for c in (1, 2, 3, 4, 5):
        t.append(('seg_loss-c%d' % c, lambda c=c: _seg_loss_case(c)))
    for c in (8, 68):
        t.append(('channel_scale-c%d' % c, lambda c=c: _channel_scale_case(c)))
        t.append(('global_avgpool-c%d' % c, lambda c=c: _global_avgpool_case(c)))
        t.append(('spade_modulate-c%d' % c, lambda c=c: _modulate_case(c)))
    t.append(('max_pool2x2', lambda: _pool_case(False)))
    t.append(('max_pool2x2_skip', lambda: _pool_case(True)))
    t.append(('max_unpool2x2', _unpool_case))
    for mode in ('bilinear', 'nearest'):
        for shape in ((2, 8, 5, 7), (1, 16, 16, 16), (1, 48, 17, 70)):
            t.append(('upsample2x_%s-%s' % (mode, 'x'.join(map(str, shape))), lambda mode=mode, shape=shape: _upsample_case(mode, shape)))
    for shp, act, res in (((2, 16, 10, 12), 'relu', True), ((3, 64, 8, 8), 'lrelu', False), ((1, 384, 4, 4), 'none', False), ((2, 8, 33, 17), 'relu', False)):
        t.append(('batch_norm_act-%s-%s' % ('x'.join(map(str, shp)), act), lambda shp=shp, act=act, res=res: _bn_case(shp, act, res)))
    t.append(('batch_norm_act-eval-res', lambda: _bn_case((2, 16, 10, 12), 'relu', True, training=False)))
    for dw in ((2, 36, 19, 23, 3, 1, 1), (1, 64, 17, 70, 5, 1, 2), (1, 16, 12, 14, 3, 2, 1), (1, 12, 14, 16, 7, 2, 3)):
        t.append(('dwconv2d-%s' % '-'.join(map(str, dw)), lambda dw=dw: _dwconv_case(*dw)))
    t.append(('concat_channels', _concat_case))
    t.append(('conv2d_sn', _conv_sn_case))
    return t


OP_TABLE = _op_table()
# ops whose kernels take whole pixel rows or dense [N][C] rows and therefore REJECT a channel slice (ValueError, nothing launched)
# (exception, the inputs whose slicing triggers it; None = any)
REJECTS_WIDE = {'add': (ValueError, None), 'channel_scale': (ValueError, {1})}


@pytest.mark.parametrize('name,make', OP_TABLE, ids=[n for n, _ in OP_TABLE])
def test_op_writes_completely_and_keeps_pad_lanes_zero(pkg, dev, guard, name, make):
    case = make()
    ref_y, dys, ref_g = _reference(case)
    y, g, _, _ = _execute(pkg, dev, guard, case, dys, _compact(pkg, dev))
    _compare(case, y, g, ref_y, ref_g, name)
    assert guard.records


SLICEABLE = [(n, m) for n, m in OP_TABLE if re.search(r'-c4$|-c8$|-c68$|^max_|^upsample|batch_norm_act-\d|batch_norm_act-eval-res|^dwconv2d|^concat|^conv2d_sn', n)]


@pytest.mark.parametrize('name,make', SLICEABLE, ids=[n for n, _ in SLICEABLE])
def test_op_on_channel_slice_inputs(pkg, dev, guard, name, make):
    case = make()
    op = name.split('-')[0]
    if op == 'global_avgpool':
        # forward takes the slice; its backward reads the pooled gradient as dense rows and rejects a wide one
        pairs = _slice_runs(pkg, dev, guard, dict(case, fwd_only=True), name)
        ref_y, dys, ref_g = _reference(case)
        v = lp.poisoned_slice(dys[0], 2 * dys[0].shape[1], 0, dev)
        x = pkg.ops.to_nhwc(case['xs'][0].to(dev)).requires_grad_(True)
        with pytest.raises(ValueError):
            pkg.ops.global_avgpool(x).backward(v)
        lp.check_slice(v)
    else:
        pairs = _slice_runs(pkg, dev, guard, case, name, expect_raise=REJECTS_WIDE.get(op))
    assert not pairs, pairs                                        # none of these ops has PROFILE labels: always bit-identical


def test_nan_to_zero_and_to_nhwc(pkg, dev, guard):
    ops = pkg.ops
    for c in ODD_CHANNELS + (8,):
        x = torch.randn(2, c, 5, 7, generator=_gen(c))
        y = ops.to_nhwc(x.to(dev))
        guard.check()
        assert y.stride() == (5 * 7 * lp.pad4(c), 1, 7 * lp.pad4(c), lp.pad4(c)) and torch.equal(y.cpu(), x)
        assert ops.to_nhwc(y) is y
        x[0, 0, 0, 0] = float('nan'); x[1, c - 1, 4, 6] = float('nan')
        xd = x.to(dev).requires_grad_(True)
        z = ops.nan_to_zero_(ops.mul(xd, torch.ones_like(xd)))     # an NHWC-with-stride tensor that is not a leaf
        guard.check()
        _no_nan(z, 'nan_to_zero_')
        want = torch.where(torch.isnan(x), torch.zeros_like(x), x)
        assert torch.equal(z.detach().cpu(), want)                  # test_seg_loss_vs_oracle: exact
        z.sum().backward()
        guard.check()
        assert torch.equal(xd.grad.cpu(), (~torch.isnan(x)).float())
    # the incoming gradient as a channel slice of a wider one (what concat_channels / add hand upstream): the mask follows x's
    # compact rows, so the backward must pick the slice's own lanes -- same bits as with a compact gradient, neighbours intact
    x = torch.randn(2, 8, 5, 7, generator=_gen(1)); x[0, 3, 2, 2] = float('nan'); x[1, 7, 4, 6] = float('nan')
    dy = torch.randn(2, 8, 5, 7, generator=_gen(2))

    def grad_for(dyd):
        xd = x.to(dev).requires_grad_(True)
        z = ops.nan_to_zero_(ops.mul(xd, torch.ones_like(xd)))
        z.backward(dyd)
        guard.check()
        return xd.grad
    g0 = grad_for(ops.to_nhwc(dy.to(dev)))
    assert torch.equal(g0.cpu(), torch.where(torch.isnan(x), torch.zeros_like(dy), dy))
    for c0, ld in _placements(8):
        v = lp.poisoned_slice(dy, ld, c0, dev)
        assert ops.nhwc_ld(v) == ld and ops.to_nhwc(v) is v
        g1 = grad_for(v)
        lp.check_slice(v)
        _no_nan(g1, 'nan_to_zero_ backward on a gradient slice')
        assert torch.equal(g1, g0), (c0, ld)
    # a channel slice as the tensor itself: whole pixel rows would be rewritten (the neighbours' NaNs zeroed, c0 floats past the
    # end touched): rejected
    for c0, ld in _placements(8):
        v = lp.poisoned_slice(x, ld, c0, dev)
        assert ops.nhwc_ld(v) == ld and ops.to_nhwc(v) is v
        with pytest.raises(ValueError):
            ops.nan_to_zero_(v)
        lp.check_slice(v)
        assert torch.isnan(v[0, 3, 2, 2]).item()


@pytest.mark.parametrize('n,k,o,act', [(2, 64, 32, True), (5, 288, 1024, True), (16, 48, 20, False), (19, 1300, 7, True), (3, 1024, 1, False)])
def test_linear_guarded_and_on_wide_rows(pkg, dev, guard, n, k, o, act):
    """test_linear's shapes and tolerances; then x as rows of a wider matrix (row stride k + 4 and 2k, first and upper half)."""
    ops = pkg.ops
    g = _gen(9)
    x = torch.randn(n, k, generator=g); wt = torch.randn(o, k, generator=g) / math.sqrt(k); b = torch.randn(o, generator=g)
    r = [t.double().requires_grad_(True) for t in (x, wt, b)]
    yr = F.linear(*r)
    if act:
        yr = F.leaky_relu(yr, 0.2)
    dy = torch.randn(yr.shape, generator=g)
    yr.backward(dy.double())

    def run(xd, dyd=None):
        d = [xd.requires_grad_(True)] + [t.to(dev).requires_grad_(True) for t in (wt, b)]
        yd = ops.linear(d[0], d[1], d[2], act=pkg._lib.ACT_LRELU if act else 0, slope=0.2)
        guard.check()
        yd.backward(dy.to(dev) if dyd is None else dyd)
        guard.check()
        return yd.detach(), [t.grad for t in d]
    y0, g0 = run(x.to(dev))
    _close(y0, yr, 1e-5, 1e-5, 'linear')
    for a, bb, nm in zip(g0, r, ('dx', 'dw', 'db')):
        _close(a, bb.grad, 2e-5, 2e-5, 'linear ' + nm)
    for c0, ld in _placements(k):
        v = lp.poisoned_slice(x.t().reshape(1, k, 1, n), ld, c0, dev)
        x2 = v.as_strided((n, k), (ld, 1), v.storage_offset())
        assert x2.stride() == (ld, 1) and torch.equal(x2.cpu(), x)
        y1, g1 = run(x2)
        lp.check_slice(v)
        for a, bb in zip([y1] + g1, [y0] + g0):
            _no_nan(a, 'linear on wide rows')
            assert torch.equal(a, bb), (c0, ld, (a - bb).abs().max().item())
    if o % 4 == 0:                                                   # the incoming gradient as rows of a wider matrix
        for c0, ld in _placements(o):
            v = lp.poisoned_slice(dy.t().reshape(1, o, 1, n), ld, c0, dev)
            d2 = v.as_strided((n, o), (ld, 1), v.storage_offset())
            assert d2.stride() == (ld, 1) and torch.equal(d2.cpu(), dy)
            y1, g1 = run(x.to(dev), d2)
            lp.check_slice(v)
            for a, bb in zip([y1] + g1, [y0] + g0):
                _no_nan(a, 'linear with a wide-row gradient')
                assert torch.equal(a, bb), ('dy', c0, ld, (a - bb).abs().max().item())


def test_se_gate_guarded_and_on_a_slice(pkg, dev, guard):
    """test_se_gate_matches_the_two_convs (tests/test_round3_gpu.py), its first shape and its bound."""
    import torch.nn as nn
    n, c, s = 4, 144, 6
    torch.manual_seed(5 + c)
    red = nn.Conv2d(c, s, 1); exp = nn.Conv2d(s, c, 1)
    sq = torch.randn(n, c, 1, 1) * 0.7
    g = torch.randn(n, c, 1, 1)
    sqr = sq.double().requires_grad_(True)
    P = [t.double().detach().requires_grad_(True) for t in (red.weight, red.bias, exp.weight, exp.bias)]
    h = F.conv2d(sqr, P[0], P[1])
    ref = torch.sigmoid(F.conv2d(h * torch.sigmoid(h), P[2], P[3]))
    ref.backward(g.double())
    red = red.to(dev); exp = exp.to(dev)

    def close(a, b, what):
        a = a.detach().cpu().double().reshape(b.shape); err = (a - b).abs().max().item(); ref_ = b.abs().max().item()
        assert err <= 2e-6 * max(ref_, 1.0) + 1e-5 * ref_, '%s: %.3e vs max %.3e' % (what, err, ref_)

    def run(sqd, gd):
        red.zero_grad(set_to_none=True); exp.zero_grad(set_to_none=True)
        sqd.requires_grad_(True)
        out = pkg.ops.se_gate(sqd, red, exp)
        assert out is not None
        guard.check()
        out.backward(gd)
        guard.check()
        return [out.detach(), sqd.grad, red.weight.grad, red.bias.grad, exp.weight.grad, exp.bias.grad]
    r0 = run(sq.to(dev), g.to(dev))
    for a, b, nm in zip(r0, [ref.detach(), sqr.grad] + [p.grad for p in P], ('gate', 'dsq', 'dw1', 'db1', 'dw2', 'db2')):
        close(a, b, nm)
    for c0, ld in _placements(c):
        vs = lp.poisoned_slice(sq, ld, c0, dev); vg = lp.poisoned_slice(g, ld, c0, dev)
        assert pkg.ops.nhwc_ld(vs) == ld and pkg.ops.to_nhwc(vs) is vs
        r1 = run(vs, vg)
        lp.check_slice(vs); lp.check_slice(vg)
        for a, b in zip(r1, r0):
            _no_nan(a, 'se_gate on a slice')
            assert torch.equal(a, b), (c0, ld)


# ----------------------------------------------------------------------------------------------------------- convolutions
def _conv_case(n, cin, cout, h, w, k, s, p, bias, act='none', res=False, c1=None, bn_stats=False, seed=None):
    """conv2d fwd + bwd; x2 = the channels from c1 on.  Tolerances: test_conv2d_fwd_bwd / test_conv2d_specialised_kernels."""
    g = _gen(1234 + cin + cout if seed is None else seed)
    x = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, k, k, generator=g) / math.sqrt(cin * k * k)
    b = torch.randn(cout, generator=g)
    oh, ow = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
    rs = torch.randn(n, cout, oh, ow, generator=g)
    fn = {'relu': F.relu, 'lrelu': lambda t: F.leaky_relu(t, 0.2), 'none': lambda t: t}[act]
    xs = ([x] if c1 is None else [x[:, :c1].contiguous(), x[:, c1:].contiguous()]) + ([rs] if res else [])
    nx = 1 if c1 is None else 2

    def dev_fn(pkg, xs, ps):
        code = {'relu': pkg._lib.ACT_RELU, 'lrelu': pkg._lib.ACT_LRELU, 'none': pkg._lib.ACT_NONE}[act]
        y = pkg.ops.conv2d(xs[0], ps[0], ps[1] if bias else None, s, p, act=code, slope=0.2, x2=xs[1] if nx == 2 else None,
                           res=xs[nx] if res else None, bn_stats=bn_stats)
        return y[0] if bn_stats else y

    def ref_fn(xs, ps):
        y = F.conv2d(torch.cat(xs[:nx], 1) if nx == 2 else xs[0], ps[0], ps[1] if bias else None, s, p)
        return fn(y + xs[nx] if res else y)
    dgrad = (1e-5, 2e-6 * math.sqrt(cout * k * k))
    return _case(xs, dev_fn, ref_fn, (1e-5, 2e-6 * math.sqrt(cin * k * k)),
                 [dgrad] * nx + ([(1e-6, 1e-6)] if res else []) + [(2e-5, 2e-6 * math.sqrt(n * h * w)), (2e-5, 1e-5) if bias else None], ps=[wt, b])


# the conv shapes of test_conv2d_fwd_bwd plus: channel counts with 3, 2 and 1 pad lanes on either side (and 66), the stride-2
# shapes of test_merged_parity_input_gradient_of_stride2_conv / test_merged_parity_declines_narrow_images, and a 1x1 stride-2
# conv (three parity classes of its input gradient have no taps: dx.zero_() is their only writer)
EDGE_CONVS = [
    (2, 1, 5, 9, 11, 3, 1, 1, True), (2, 2, 6, 10, 9, 3, 1, 1, False), (1, 5, 7, 12, 13, 3, 1, 1, True), (2, 6, 1, 8, 9, 1, 1, 0, True),
    (1, 7, 2, 11, 10, 3, 2, 1, False), (2, 3, 3, 9, 9, 3, 1, 1, True), (2, 66, 66, 9, 10, 3, 1, 1, True), (2, 64, 5, 16, 16, 3, 1, 1, True),
    (2, 66, 7, 12, 12, 1, 1, 0, False), (1, 6, 66, 10, 12, 3, 1, 1, True), (2, 1, 1, 7, 9, 3, 1, 1, True), (2, 2, 2, 8, 8, 3, 2, 1, True),
    (2, 16, 24, 15, 17, 1, 2, 0, True), (2, 3, 5, 16, 18, 1, 2, 0, False), (1, 64, 64, 31, 33, 1, 2, 0, False),
    (3, 64, 64, 96, 128, 3, 2, 1, False), (2, 128, 256, 63, 65, 3, 2, 1, False), (2, 192, 64, 34, 40, 3, 2, 1, True), (1, 64, 48, 31, 33, 3, 2, 1, False),
    (2, 64, 64, 24, 30, 3, 2, 1, False),
]
# 3x3 stride-2 pad-1 shapes: the input gradient is ONE parity-merged launch, or four per-class launches where dy is narrower than 17
PARITY_LAUNCHES = {(3, 64, 64, 96, 128, 3, 2, 1, False): 'merged', (2, 128, 256, 63, 65, 3, 2, 1, False): 'merged',
                   (2, 192, 64, 34, 40, 3, 2, 1, True): 'merged', (1, 64, 48, 31, 33, 3, 2, 1, False): 'merged',
                   (2, 64, 64, 24, 30, 3, 2, 1, False): 'classes'}
VARIANTS = ('plain', 'relu+res', 'lrelu', 'bn_stats', 'x2+res')


def _variant(case, variant):
    n, cin, cout, h, w, k, s, p, bias = case
    if variant == 'plain':
        return _conv_case(*case)
    if variant == 'relu+res':
        return _conv_case(*case, act='relu', res=True)
    if variant == 'lrelu':
        return _conv_case(*case, act='lrelu')
    if variant == 'bn_stats':
        return _conv_case(*case, bn_stats=True)
    return _conv_case(*case, res=True, c1=cin // 8 * 4)




def _outputs(c):
    n, cin, cout, h, w, k, s, p, bias = c
    return n * cout * ((h + 2 * p - k) // s + 1) * ((w + 2 * p - k) // s + 1)


# An activation's mask is discontinuous: a pre-activation within fp32 rounding (~1e-6 of values of order 1, a 4e-7 chance per
# output) has another sign in fp64 and moves the gradient by slope * dy * w.  The activation variants therefore run on the shapes
# with fewer than 1e5 outputs (test_conv2d_specialised_kernels draws the same line at 1e6 against an fp32 reference); the two large
# stride-2 shapes keep the variants without a mask.
CONV_RUNS = [(c, v) for c in CONV_CASES + EDGE_CONVS for v in VARIANTS
             if (v != 'x2+res' or c[1] >= 8) and (v not in ('relu+res', 'lrelu') or _outputs(c) < 100000)]


@pytest.mark.parametrize('case,variant', CONV_RUNS, ids=['%s-%s' % ('x'.join(map(str, c[:8])), v) for c, v in CONV_RUNS])
def test_conv2d_writes_completely(pkg, dev, guard, case, variant):
    cs = _variant(case, variant)
    ref_y, dys, ref_g = _reference(cs)
    y, g, labels, _ = _execute(pkg, dev, guard, cs, dys, _compact(pkg, dev))
    _compare(cs, y, g, ref_y, ref_g, '%s %s %s' % (case, variant, labels))
    assert guard.records
    if case in PARITY_LAUNCHES and variant != 'x2+res':             # which kernel wrote dx (test_split_gpu.py pins the same)
        merged = [l for l in labels if l == 'conv_igemm_halo_x3_kernel<128,64,4,1,true>']
        if PARITY_LAUNCHES[case] == 'merged':
            assert len(merged) == 1 and len(labels) == 3, labels    # forward, one merged input gradient, weight gradient
        else:
            assert not merged and len(labels) == 6, labels          # forward, four per-class launches, weight gradient


def _family_runs():
    """(case, family, expected labels) of test_conv2d_specialised_kernels, without the combinations it skips."""
    runs = []
    for case in KERNEL_CASES:
        n, cin, cout, h, w, k, p, expect = case
        for family in ('x3', 'fp32mfma', 'k32'):
            exp = expect
            if family == 'x3':
                if not any(_split_label(e) != e for e in expect):
                    continue
                exp = tuple(_split_label(e) if (cout % 64 == 0 or e.startswith('wgrad')) else e for e in expect)
            elif family == 'k32':
                swap = [_k32_label(e, cin, cout, w) for e in expect]
                if not any(swap) or not (cin % 64 == 0 and cout % 64 == 0):
                    continue
                exp = tuple(sw if sw else _split_label(e) for e, sw in zip(expect, swap))
            runs.append((case[:7], family, exp))
    return runs


FAMILY_RUNS = _family_runs()
# test_narrow_k32_tiles: (c1, c2, co, h, w, nb), forced onto the k32 kernels
NARROW_K32 = [(512, 0, 16, 64, 64, 4), (256, 0, 24, 40, 72, 3), (128, 128, 32, 33, 50, 2), (128, 0, 12, 24, 40, 2)]
_REF_CACHE = {}


class _forced(object):
    """The forcing of test_conv2d_specialised_kernels: k32 modes through the library switches, MFMA_SPLIT through monkeypatch."""

    def __init__(self, pkg, monkeypatch, family):
        self.pkg, self.mp, self.family = pkg, monkeypatch, family

    def __enter__(self):
        self.pkg._lib.call('ssg_conv_set_k32_mode', 2 if self.family == 'k32' else 0)
        self.pkg._lib.call('ssg_wgrad_set_k32_mode', 1 if self.family == 'k32' else 0)
        self.mp.setattr(self.pkg.ops, 'MFMA_SPLIT', self.family != 'fp32mfma')

    def __exit__(self, *a):
        self.pkg._lib.call('ssg_conv_set_k32_mode', 1); self.pkg._lib.call('ssg_wgrad_set_k32_mode', 1)


def _has(labels, name):
    return any(l == name or (name.endswith('<') and l.startswith(name)) for l in labels)


@pytest.mark.parametrize('case,family,expect', FAMILY_RUNS, ids=['%s-%s' % ('x'.join(map(str, c)), f) for c, f, _ in FAMILY_RUNS])
def test_specialised_conv_kernels_write_completely(pkg, dev, guard, monkeypatch, case, family, expect):
    n, cin, cout, h, w, k, p = case
    use_act = n * h * w * cout < 1000000                            # test_conv2d_specialised_kernels: mask flips on the one large case
    cs = _conv_case(n, cin, cout, h, w, k, 1, p, True, act='lrelu' if use_act else 'none', res=True)
    if case not in _REF_CACHE:
        torch.set_num_threads(16)
        _REF_CACHE[case] = _reference(cs)
    ref_y, dys, ref_g = _REF_CACHE[case]
    with _forced(pkg, monkeypatch, family):
        y, g, labels, _ = _execute(pkg, dev, guard, cs, dys, _compact(pkg, dev))
    for name in expect:
        assert _has(labels, name), '%s did not run (ran: %s)' % (name, labels)
    _compare(cs, y, g, ref_y, ref_g, '%s %s' % (case, family))


@pytest.mark.parametrize('c1,c2,co,h,w,nb', NARROW_K32)
def test_narrow_k32_tiles_write_completely(pkg, dev, guard, monkeypatch, c1, c2, co, h, w, nb):
    cs = _conv_case(nb, c1 + c2, co, h, w, 3, 1, 1, True, act='lrelu', res=True, c1=c1 if c2 else None, seed=31)
    torch.set_num_threads(16)
    ref_y, dys, ref_g = _reference(cs)
    with _forced(pkg, monkeypatch, 'k32'):
        y, g, labels, _ = _execute(pkg, dev, guard, cs, dys, _compact(pkg, dev))
    assert ('k32_kernel<8,16>' if co <= 16 else 'k32_kernel<8,32>') in labels[0], labels
    _compare(cs, y, g, ref_y, ref_g, 'narrow k32 %s' % labels)


# one shape per conv family for the channel-slice inputs (n, cin, cout, h, w, k, s, p, family, c1 of a two-input conv or None)
SLICE_CONVS = [
    (2, 16, 32, 20, 24, 3, 1, 1, 'x3', 8), (1, 64, 64, 32, 32, 3, 1, 1, 'x3', None), (1, 64, 64, 32, 32, 3, 1, 1, 'fp32mfma', 32),
    (1, 64, 64, 32, 32, 3, 1, 1, 'k32', None), (2, 32, 48, 16, 16, 1, 1, 0, 'x3', None), (2, 16, 16, 16, 16, 3, 2, 1, 'x3', None),
    (3, 64, 64, 96, 128, 3, 2, 1, 'x3', None), (1, 256, 256, 16, 16, 3, 1, 1, 'x3', None), (2, 256, 256, 12, 14, 3, 1, 1, 'x3', None),
    (2, 4, 64, 37, 45, 3, 1, 1, 'x3', None), (1, 128, 4, 19, 23, 3, 1, 1, 'x3', None), (1, 4, 8, 19, 70, 3, 1, 1, 'x3', None),
    (1, 64, 96, 256, 257, 1, 1, 0, 'x3', None), (1, 4, 96, 260, 270, 3, 1, 1, 'x3', None), (2, 64, 128, 37, 45, 3, 1, 1, 'fp32mfma', None),
    (2, 64, 128, 37, 45, 3, 1, 1, 'k32', 32), (2, 48, 80, 14, 14, 1, 1, 0, 'fp32mfma', None), (2, 128, 32, 33, 50, 3, 1, 1, 'k32', None),
]
# (compact labels, wide-stride labels) where the launch plan legitimately picks another kernel for a wide pixel stride
WIDE_STRIDE_SWITCH = set()


@pytest.mark.parametrize('spec', SLICE_CONVS, ids=['%s-%s' % ('x'.join(map(str, s[:8])), s[8]) for s in SLICE_CONVS])
def test_conv2d_on_channel_slice_inputs(pkg, dev, guard, monkeypatch, spec):
    n, cin, cout, h, w, k, s, p, family, c1 = spec
    cs = _conv_case(n, cin, cout, h, w, k, s, p, True, act='none', res=True, c1=c1)
    with _forced(pkg, monkeypatch, family):
        pairs = _slice_runs(pkg, dev, guard, cs, 'conv %s' % (spec,), switch=WIDE_STRIDE_SWITCH)
    print('wide-stride label pairs %s: %s' % (spec, sorted(pairs)))


# ----------------------------------------------------------------------------------------------------------- destination slices
# (n, cin, cout, h, w, k, p, forcing, label that must run): one per conv family behind _conv_fwd_impl(..., out=)
DEST_CONVS = [
    (2, 4, 64, 37, 45, 3, 1, 'x3', 'thin4_cin_kernel'), (1, 128, 4, 19, 23, 3, 1, 'x3', 'thin4_cout_kernel'), (1, 4, 8, 19, 70, 3, 1, 'x3', 'tiny4_kernel'),
    (1, 4, 96, 260, 270, 3, 1, 'x3', 'thin32_cin_kernel'),
    (2, 64, 128, 37, 45, 3, 1, 'fp32mfma', 'conv_igemm_halo_kernel<128,64>'), (2, 64, 128, 16, 16, 3, 1, 'fp32mfma', 'conv_igemm_halo16_kernel<128,128>'),
    (2, 256, 256, 12, 14, 3, 1, 'fp32mfma', 'conv_igemm_halo16_kernel<128,128>+splitk'), (1, 512, 96, 20, 40, 3, 1, 'fp32mfma', 'conv_igemm_halo_kernel<128,64>+splitk'),
    (2, 48, 80, 14, 14, 1, 0, 'fp32mfma', 'conv_igemm_dma_kernel<128,64>'), (1, 320, 80, 14, 14, 1, 0, 'fp32mfma', 'conv_igemm_dma_kernel<128,128>'),
    (1, 64, 96, 256, 257, 1, 0, 'x3', 'conv1x1_k64_kernel'), (2, 16, 32, 20, 24, 3, 1, 'x3', 'conv_igemm_kernel<'),
    (2, 64, 128, 37, 45, 3, 1, 'x3', 'conv_igemm_halo_x3_kernel<'), (4, 128, 128, 64, 64, 1, 0, 'x3', 'conv_igemm_dma_x3_kernel<128>'),
    (4, 64, 64, 48, 64, 3, 1, 'k32', 'conv_halo_k32_kernel<16,64>'), (2, 128, 128, 40, 72, 3, 1, 'k32', 'conv_halo_k32_kernel<8,128>'),
    (4, 512, 16, 64, 64, 3, 1, 'k32', 'conv_halo_k32_kernel<8,16>'), (3, 256, 24, 40, 72, 3, 1, 'k32', 'conv_halo_k32_kernel<8,32>'),
    (2, 128, 12, 24, 40, 3, 1, 'k32', 'conv_halo_k32_kernel<8,16>'),
]


@pytest.mark.parametrize('spec', DEST_CONVS, ids=['%s-%s' % ('x'.join(map(str, s[:7])), s[7]) for s in DEST_CONVS])
def test_conv_into_a_destination_slice(pkg, dev, guard, monkeypatch, spec):
    """_conv_fwd_impl(..., out=) with `out` a channel slice of a guarded canary buffer: both halves of a 2 * Cout buffer and the
    middle of a Cout + 8 one.  The slice must be completely written, its neighbours and the guards untouched, the values fp64's."""
    ops = pkg.ops
    n, cin, cout, h, w, k, p, family, label = spec
    g = _gen(cin * 7 + cout)
    x = torch.randn(n, cin, h, w, generator=g); wt = torch.randn(cout, cin, k, k, generator=g) / math.sqrt(cin * k * k)
    b = torch.randn(cout, generator=g); rs = torch.randn(n, cout, h, w, generator=g)
    torch.set_num_threads(16)
    ref = F.leaky_relu(F.conv2d(x.double(), wt.double(), b.double(), 1, p) + rs.double(), 0.2)
    xd = ops.to_nhwc(x.to(dev)); wd = wt.to(dev); bd = b.to(dev); rd = ops.to_nhwc(rs.to(dev))
    with _forced(pkg, monkeypatch, family):
        for c0, ld in ((0, 2 * cout), (cout, 2 * cout), (4, cout + 8)):
            out = lp.canary_slice(n, cout, h, w, ld, c0, dev)
            assert ops.nhwc_ld(out) == ld
            ops.PROFILE = []
            try:
                y = ops._conv_fwd_impl(xd, None, wd, bd, 1, p, pkg._lib.ACT_LRELU, 0.2, res=rd, out=out)
                labels = [r[0] for r in ops.PROFILE]
            finally:
                ops.PROFILE = None
            assert y is out and _has(labels, label), labels
            lp.check_slice(out, written=True)
            guard.check()
            _no_nan(out, 'destination slice')
            _close(out, ref, 1e-5, 2e-6 * math.sqrt(cin * k * k), 'conv into lanes [%d, %d) of %d (%s)' % (c0, c0 + cout, ld, labels))


# the `mis` rows of tests/test_conv_plan.py: the three kernels the plan pins for a destination 4 bytes off a 16-byte boundary with an odd
# pixel stride (n, cin, cout, h, w, k, p, label)
MIS_CONVS = [(2, 64, 128, 37, 45, 3, 1, 'conv_igemm_halo_x3_kernel<128,64>'), (2, 16, 32, 20, 24, 3, 1, 'conv_igemm_kernel<256,32>'),
             (4, 128, 128, 64, 64, 1, 0, 'conv_igemm_dma_x3_kernel<128>')]


@pytest.mark.parametrize('spec', MIS_CONVS, ids=[s[7] for s in MIS_CONVS])
def test_conv_into_a_misaligned_odd_stride_destination(pkg, dev, guard, monkeypatch, spec):
    """ssg_conv_desc.ldo with out 4 bytes off a 16-byte boundary and ldo = pad4(Cout) + 1 (the `mis` geometry of
    tests/test_conv_plan.py).  Such a tensor is not NHWC-with-stride, so ops._ld refuses it (pinned first); the library's launch
    is then reached through the same _conv_fwd_impl with _ld answering the destination's real stride, and its stores are checked
    like any destination slice: every element written, every other float of the buffer and both guards still the canary, fp64 values."""
    ops = pkg.ops
    n, cin, cout, h, w, k, p, label = spec
    g = _gen(cin * 11 + cout)
    x = torch.randn(n, cin, h, w, generator=g); wt = torch.randn(cout, cin, k, k, generator=g) / math.sqrt(cin * k * k)
    b = torch.randn(cout, generator=g); rs = torch.randn(n, cout, h, w, generator=g)
    ref = F.leaky_relu(F.conv2d(x.double(), wt.double(), b.double(), 1, p) + rs.double(), 0.2)
    xd = ops.to_nhwc(x.to(dev)); wd = wt.to(dev); bd = b.to(dev); rd = ops.to_nhwc(rs.to(dev))
    ldo = lp.pad4(cout) + 1
    host = lp.canary_slice(n, cout + 4, h, w, cout + 4, 0, dev)     # n*h*w*(cout + 4) floats between two guards: room for 1 + n*h*w*ldo
    rec = host._layout_probe
    out = torch.empty(0, device=dev, dtype=torch.float32).set_(rec.buf.untyped_storage(), rec.guard + 1, (n, cout, h, w), (h * w * ldo, 1, w * ldo, ldo))
    assert ops.nhwc_ld(out) is None and out.data_ptr() % 16 == 4
    with pytest.raises(pkg._lib.HipLibraryError):
        ops._conv_fwd_impl(xd, None, wd, bd, 1, p, pkg._lib.ACT_LRELU, 0.2, res=rd, out=out)
    torch.cuda.synchronize()
    assert bool(lp.is_canary(rec.buf).all())                         # refused before anything was launched
    real_ld = ops._ld
    monkeypatch.setattr(ops, '_ld', lambda t: ldo if t is out else real_ld(t))
    with _forced(pkg, monkeypatch, 'x3'):
        ops.PROFILE = []
        try:
            y = ops._conv_fwd_impl(xd, None, wd, bd, 1, p, pkg._lib.ACT_LRELU, 0.2, res=rd, out=out)
            labels = [r[0] for r in ops.PROFILE]
        finally:
            ops.PROFILE = None
    assert y is out and labels == [label], labels
    torch.cuda.synchronize()
    own = torch.zeros(rec.buf.numel(), dtype=torch.bool, device=dev)
    idx = (rec.guard + 1 + torch.arange(n * h * w, device=dev)[:, None] * ldo + torch.arange(cout, device=dev)[None, :]).reshape(-1)
    own[idx] = True
    still = lp.is_canary(rec.buf)
    assert int((still & own).sum()) == 0, '%d elements of the destination never written' % int((still & own).sum())
    stray = (~still) & (~own)
    assert int(stray.sum()) == 0, '%d floats outside the destination overwritten, first at float %d of the buffer (payload starts at %d)' % (
        int(stray.sum()), int(stray.nonzero()[0]), rec.guard)
    guard.check()
    _no_nan(out, 'misaligned destination')
    _close(out, ref, 1e-5, 2e-6 * math.sqrt(cin * k * k), 'conv into a misaligned destination (%s)' % labels)


# ----------------------------------------------------------------------------------------------------------- composite paths
def _spade_reference(m, x, dy):
    P = {k: v.detach().cpu().double().requires_grad_(True) for k, v in m.named_parameters()}
    xr = x.double().requires_grad_(True)
    seg = F.conv2d(xr, P['x2map.weight'], P['x2map.bias'], 1, 1)
    a = F.relu(F.conv2d(seg, P['mlp_shared.0.weight'], P['mlp_shared.0.bias'], 1, 1))
    gam = F.conv2d(a, P['mlp_gamma.weight'], P['mlp_gamma.bias'], 1, 1); bet = F.conv2d(a, P['mlp_beta.weight'], P['mlp_beta.bias'], 1, 1)
    yr = xr * (1 + gam) + bet
    yr.backward(dy.double())
    return yr.detach(), xr.grad, P


@pytest.mark.parametrize('c,h,w,fused', [(64, 256, 257, True), (128, 130, 515, True), (64, 20, 27, False), (128, 12, 13, False)])
def test_spade_self_writes_completely(pkg, dev, guard, c, h, w, fused):
    """blocks.spade_self on the fused thin32_cin<spade> route and on the two-kernel route, bounds of
    test_spade_fused_gamma_beta_modulate (tests/test_blocks_gpu.py); then with x and dy as channel slices."""
    torch.manual_seed(21)
    m = pkg.normalization.SPADE('spadebatch3x3', c, 3, c / 16).to(dev).train()
    g = _gen(5)
    x = torch.randn(1, c, h, w, generator=g); dy = torch.randn(1, c, h, w, generator=g)
    torch.set_num_threads(16)
    yr, dxr, P = _spade_reference(m, x, dy)

    def close(got, ref, nm, rtol=2e-5):
        e = (got.detach().cpu().double() - ref).abs().max().item()
        assert e <= rtol * ref.abs().max().item() + 1e-6, '%s: max err %.3e (ref max %.3e)' % (nm, e, ref.abs().max().item())

    def run(xd, dyd):
        m.zero_grad(set_to_none=True)
        xd.requires_grad_(True)
        pkg.ops.PROFILE = []
        try:
            yd = m(xd, xd)
            guard.check()
            yd.backward(dyd)
            guard.check()
            labels = [r[0] for r in pkg.ops.PROFILE]
        finally:
            pkg.ops.PROFILE = None
        return [yd.detach(), xd.grad] + [v.grad for _, v in m.named_parameters()], labels
    r0, l0 = run(pkg.ops.to_nhwc(x.to(dev)), dy.to(dev))
    assert ('thin32_cin_kernel<spade>' in l0) == fused, l0
    close(r0[0], yr, 'out'); close(r0[1], dxr, 'dx', 5e-5)
    for (k, v), got in zip(m.named_parameters(), r0[2:]):
        close(got, P[k].grad, k, 2e-4)
    assert {'_spade_fused_fwd' if fused else '_conv_fwd_impl', 'backward', '_act_bwd', '_conv_dgrad_impl'} <= set(guard.frames()), guard.frames()
    for c0, ld in _placements(c)[1:3]:
        vx = lp.poisoned_slice(x, ld, c0, dev); vd = lp.poisoned_slice(dy, ld, c0, dev)
        r1, l1 = run(vx, vd)
        lp.check_slice(vx); lp.check_slice(vd)
        assert l1 == l0, (l0, l1)
        for a, b in zip(r1, r0):
            _no_nan(a, 'spade on slices')
            assert torch.equal(a, b), (c0, ld, (a - b).abs().max().item())


@pytest.mark.parametrize('cin,cout,h,w,nb', [(64, 64, 48, 64, 4), (64, 128, 33, 50, 3), (16, 24, 12, 13, 2)])
def test_basic_block_writes_completely(pkg, dev, guard, monkeypatch, cin, cout, h, w, nb):
    """archs.BasicBlock forward and backward with SSG_BN_FUSE_INPUT off and on (test_basic_block_bn_apply_fused_into_conv2's forcing
    and its bounds: same bits on both routes, forward within 1e-4 of stock arithmetic -- here fp64 on the CPU)."""
    ops = pkg.ops
    torch.manual_seed(5)
    m = pkg.archs.BasicBlock(cin, cout).to(dev).train()
    with torch.no_grad():
        m.bn1.bias.fill_(0.7); m.bn1.weight.uniform_(0.5, 1.5)
    x0 = torch.randn(nb, cin, h, w, device=dev); dy = torch.randn(nb, cout, h, w, device=dev)
    state = {k: v.clone() for k, v in m.state_dict().items()}
    outs = {}
    with _forced(pkg, monkeypatch, 'k32'):
        for fused in (False, True):
            m.load_state_dict(state)
            monkeypatch.setattr(ops, 'BN_FUSE_INPUT', fused)
            x = x0.clone().requires_grad_(True)
            m.zero_grad(set_to_none=True)
            y = m(x)
            guard.check()
            y.backward(dy)
            guard.check()
            outs[fused] = [y.detach().clone(), x.grad.clone()] + [p.grad.clone() for p in m.parameters()]
    for a, b in zip(outs[True], outs[False]):
        _no_nan(a, 'basic block')
        assert torch.equal(a, b), (a - b).abs().max().item()
    sd = {k: v.cpu().double() for k, v in state.items()}
    xr = x0.cpu().double()
    c1 = F.conv2d(xr, sd['conv1.weight'], None, 1, 1)
    y1 = F.relu(F.batch_norm(c1, None, None, sd['bn1.weight'], sd['bn1.bias'], True, 0.1, 1e-5))
    o = F.batch_norm(F.conv2d(y1, sd['conv2.weight'], None, 1, 1), None, None, sd['bn2.weight'], sd['bn2.bias'], True, 0.1, 1e-5)
    o = F.relu(o + (F.conv2d(xr, sd['shortcut.0.weight'], None, 1, 0) if 'shortcut.0.weight' in sd else xr))
    err = (outs[True][0].cpu().double() - o).abs().max().item()
    assert err <= 1e-4 * max(1.0, o.abs().max().item()), err
    assert {'_conv_fwd_impl', '_bn_apply', '_bn_bwd_body', '_conv_dgrad_impl'} <= set(guard.frames()), guard.frames()


def test_bf16_entry_points_write_completely(pkg, dev, guard):
    """The bf16 family's fp32 boundary tensors come from ops.new_nhwc: the stem's image gradient (3 channels: one pad lane), to_f32
    behind the GEMM, the pooled vector and the gate gradient.  Bounds: test_stem_conv_bf16 / test_gemm_bf16_fwd."""
    bf = pkg.bf16
    g = _gen(3)
    for n, cin, h, w, co, k, stride, pad in ((2, 3, 37, 50, 32, 3, 2, (0, 1, 0, 1)), (1, 4, 20, 24, 40, 5, 2, (1, 2, 1, 2))):
        x = torch.randn(n, cin, h, w, generator=g); wt = torch.randn(co, cin, k, k, generator=g) / (k * cin ** 0.5)
        pt, pb, pl, pr = pkg.ops._pad4(pad)
        xp = F.pad(x.bfloat16().double(), (pl, pr, pt, pb)).requires_grad_(True); wr = wt.bfloat16().double().requires_grad_(True)
        ref = F.conv2d(xp, wr, None, stride)
        xd = x.to(dev).requires_grad_(True); wd = wt.to(dev).requires_grad_(True)
        y = bf.conv_thin(xd, wd, stride, pad)
        guard.check()
        err = (y.double().cpu() - ref.detach()).abs()
        assert (err <= 2.0 ** -8 * ref.detach().abs() + 1e-6).all(), err.max().item()
        dy = torch.randn(ref.shape, generator=g).bfloat16()
        y.backward(dy.to(dev))
        guard.check()
        ref.backward(dy.double())
        dxr = xp.grad[:, :, pt:pt + h, pl:pl + w]
        assert (wd.grad.double().cpu() - wr.grad).abs().max().item() <= 1e-4 * max(1.0, wr.grad.abs().max().item())
        assert (xd.grad.double().cpu() - dxr).abs().max().item() <= 1e-4 * max(1.0, dxr.abs().max().item())
    # GEMM (1x1 conv) between the two dtype boundaries, then the pooled vector and the gate
    x = torch.randn(2, 24, 9, 13, generator=g); wt = torch.randn(144, 24, 1, 1, generator=g) / 24 ** 0.5
    xd = x.to(dev).requires_grad_(True); wd = wt.to(dev).requires_grad_(True)
    yb = bf.conv1x1(bf.to_bf16(xd), wd)
    y = bf.to_f32(yb)
    guard.check()
    r = F.conv2d(x.bfloat16().float(), wt.bfloat16().float())
    err = (y.detach().cpu() - r).abs()
    assert not torch.isnan(y).any() and (err <= 2 ** -8 * r.abs() + 1e-3).all(), err.max().item()
    pooled = bf.global_avgpool(yb)
    guard.check()
    assert pooled.dtype == torch.float32 and tuple(pooled.shape) == (2, 144, 1, 1)
    gate = torch.rand(2, 144, 1, 1, generator=g).to(dev).requires_grad_(True)
    z = bf.channel_scale(yb, gate)
    (bf.to_f32(z).sum() + y.sum() + pooled.sum()).backward()
    guard.check()
    assert {'_to_f32_impl', 'forward', 'backward'} <= set(guard.frames()), guard.frames()
    _no_nan(xd.grad, 'bf16 dx'); _no_nan(gate.grad, 'bf16 dgate')


# ----------------------------------------------------------------------------------------------------------- meta
# ops with a test of their own here instead of a row in OP_TABLE
DEDICATED = {'conv2d': 'test_conv2d_writes_completely', 'linear': 'test_linear_guarded_and_on_wide_rows',
             'se_gate': 'test_se_gate_guarded_and_on_a_slice', 'nan_to_zero_': 'test_nan_to_zero_and_to_nhwc',
             'to_nhwc': 'test_nan_to_zero_and_to_nhwc'}


def test_every_public_op_is_exercised_or_exempt(pkg):
    """Every name of ops.__all__ and the four public ops it leaves out has a row in OP_TABLE (each row runs under the guards, the
    sliceable ones again on channel slices) or a dedicated test here, or is in EXEMPT because it neither takes nor produces an
    NHWC tensor."""
    assert set(EXEMPT) == {'bump_weight_epoch', 'spectral_norm_weight', 'bce_with_logits_const', 'new_nhwc'}
    table_ops = set(n.split('-')[0] for n, _ in OP_TABLE)
    for name, test in DEDICATED.items():
        assert callable(globals().get(test)) and callable(getattr(pkg.ops, name)), (name, test)
    for n in list(pkg.ops.__all__) + list(EXTRA_PUBLIC):
        assert callable(getattr(pkg.ops, n)), n
        assert (n in EXEMPT) != (n in table_ops or n in DEDICATED), '%s: neither exercised nor exempt (or both)' % n
    for row in table_ops:
        assert row in pkg.ops.__all__ or row in EXTRA_PUBLIC, row
