"""ssg_conv2d_bf16x2_f32 / ssg_pack_weights_bf16x2 (csrc/conv_halo_k32_bf16.hip, kernel ids 90 / 91) through the C-ABI: the two-term
3x3 stride-1 pad-1 convolution, forward and input gradient, against tests/bf16x2_ref.py (rehearsed in tests/test_bf16x2_ref.py).

Per case, with bias + residual + activation in the epilogue and every pixel stride wider than its channels (operands and the
destination are channel slices of canary-filled, guarded buffers):
  (1) small integers in both operands                         -> equal to fp64, element for element;
  (2) 12-bit integers on one side, integers in [-2, 2] on the other, both ways round (every 12-bit integer is v1 + v2 exactly,
      all partial sums stay below 2^24)                       -> equal to fp64; a one-term kernel or one without that side's cross
      product cannot be;
  (3) N(0, 1) data, N(0, 1) / sqrt(K) weights                 -> within the fp32-accumulation gate of the quantised reference, and
      within that gate + (3 * 2^-16 + 3 * 2^-32) conv(|x|, |w|) of the exact one;
  (4) +inf, NaN, 3.39e38 (infinite in bf16) in x and in w     -> the NaN / inf / finite pattern of the fp32-class kernel on the same
      call, finite values within the gate of (3).
The route is asserted through ssg_conv2d_bf16x2_kernel_id; the pack is compared byte for byte with bf16x2_ref.pack_x2; refusals
return a status and launch nothing."""
import ctypes as C

import numpy as np
import pytest
import torch

import bf16x2_ref as R
import layout_probe as LP

pytestmark = pytest.mark.gpu


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _launch_fwd(pkg, x1, x2, wd, bias, res, out, code, slope, family='bf16x2'):
    """One ssg_conv2d_bf16x2_f32 launch as ops._conv_bf16x1_impl builds it, with the route asserted; returns the kernel id.
    family='bf16x1': the one-term entry points on the same descriptor (format codes 1128 / 1064)."""
    ops, lib = pkg.ops, pkg._lib
    d = ops._x1_desc(x1, x2, wd, res, out)
    wpk, kp, kmode = ops._pack(wd, 0, ops._X1_TAPS, wd.shape[1], x1.shape[1])
    d.w = wpk.data_ptr(); d.Kp = kp; d.kmode = kmode
    d.bias = bias.data_ptr() if bias is not None else None
    d.act = code; d.slope = slope
    fmt = lib.call('ssg_conv2d_%s_ok' % family, C.byref(d))
    assert fmt == (2000 if family == 'bf16x2' else 1000) + (128 if wd.shape[0] % 128 == 0 else 64), fmt
    kid = lib.call('ssg_conv2d_%s_kernel_id' % family, C.byref(d))
    pack = ops._x1_pack(wd, wpk, kp, fmt, family=family)
    lib.call('ssg_conv2d_%s_f32' % family, C.byref(d), ops.ptr(pack), ops.stream_ptr())
    return kid


def _launch_dgrad(pkg, dy, wd, c_lo, c_hi, res, out):
    """The input gradient for input channels [c_lo, c_hi) as ops._conv_dgrad_bf16x1_impl builds it: the conv on dy with rows
    [c_lo, c_hi) of the transposed pack and the mirrored taps."""
    ops, lib = pkg.ops, pkg._lib
    o, rows = wd.shape[0], c_hi - c_lo
    d = ops._x1_desc(dy, None, wd, res, out)
    d.Cout = rows
    ops._fill_taps(d, ops._X1_TAPS_T)
    wpk, kp, kmode = ops._pack(wd, 1, ops._X1_TAPS_T, o, o)
    d.w = wpk.data_ptr() + c_lo * kp * 4; d.Kp = kp; d.kmode = kmode
    fmt = lib.call('ssg_conv2d_bf16x2_ok', C.byref(d))
    assert fmt == (2128 if rows % 128 == 0 else 2064), fmt
    kid = lib.call('ssg_conv2d_bf16x2_kernel_id', C.byref(d))
    pack = ops._x1_pack(wd, wpk, kp, fmt, transpose=1, row0=c_lo, rows=rows, family='bf16x2')
    lib.call('ssg_conv2d_bf16x2_f32', C.byref(d), ops.ptr(pack), ops.stream_ptr())
    return kid


def _data(kind, xs, ws, g, K):
    if kind == 'ints':
        return R.small_ints(xs, g), R.small_ints(ws, g), True
    if kind == 'x12':
        return R.ints12(xs, g), R.small_ints(ws, g, 2), True
    if kind == 'w12':
        return R.small_ints(xs, g, 2), R.ints12(ws, g), True
    return R.normal(xs, g), R.normal(ws, g, K ** -0.5), False


def _judge(tag, got, x, w, bias, res, act, slope, exact_class, K, e):
    """The asserts of classes (1)-(3) on a result `got` (fp64, CPU) of act(conv(x, w) + bias + res)."""
    exact = R.conv_exact(x, w, bias, res, act, slope)
    if exact_class:
        assert R.conv_mag(x, w).max().item() + 8 < 2 ** 24
        bad = (got != exact).nonzero()
        assert not len(bad), '%s: %d elements differ from fp64, first %s: %r != %r' % (
            tag, len(bad), tuple(bad[0].tolist()), got[tuple(bad[0])].item(), exact[tuple(bad[0])].item())
        return
    quant = R.conv_quant(x, w, bias, res, act, slope)
    mag = R.conv_mag(x, w)
    magt = mag + (bias.double().abs().view(1, -1, 1, 1) if bias is not None else 0) + (res.double().abs() if res is not None else 0)
    gate = R.conv_acc_gate(K, mag, quant, e, magt)
    rq = ((got - quant).abs() / gate).max().item()
    re = ((got - exact).abs() / (gate + R.BOUND * mag)).max().item()
    print('RATIO %s K=%d: |got - quantised| / gate max %.4f; |got - exact| / (gate + bound) max %.4f; |got - exact| / bound max %.4f'
          % (tag, K, rq, re, ((got - exact).abs() / (R.BOUND * mag)).max().item()))
    assert rq <= 1 and re <= 1, (rq, re)


@pytest.mark.parametrize('kind', ['ints', 'x12', 'w12', 'normal'])
@pytest.mark.parametrize('name', sorted(R.FWD_CASES))
def test_forward(pkg, dev, name, kind):
    ops = pkg.ops
    n, c1, c2, co, h, w, act, code, slope = R.FWD_CASES[name]
    K = 9 * (c1 + c2)
    g = _g(100 + len(name) + len(kind))
    x, wt, exact_class = _data(kind, (n, c1 + c2, h, w), (co, c1 + c2, 3, 3), g, K)
    bias = R.small_ints((co,), g) if exact_class else R.normal((co,), g)
    res = R.small_ints((n, co, h, w), g) if exact_class else R.normal((n, co, h, w), g)
    xs1 = LP.poisoned_slice(x[:, :c1].contiguous(), c1 + 32, 16, dev)
    xs2 = LP.poisoned_slice(x[:, c1:].contiguous(), c2 + 16, 8, dev) if c2 else None
    rs = LP.poisoned_slice(res, co + 16, 8, dev)
    out = LP.canary_slice(n, co, h, w, co + 8, 4, dev)
    assert ops.nhwc_ld(xs1) == c1 + 32 and ops.nhwc_ld(rs) == co + 16 and ops.nhwc_ld(out) == co + 8
    kid = _launch_fwd(pkg, xs1, xs2, wt.to(dev), bias.to(dev), rs, out, code, slope)
    assert kid == (90 if co % 128 == 0 else 91)
    for t in (xs1, xs2, rs):
        if t is not None:
            LP.check_slice(t)
    LP.check_slice(out, written=True)
    e = 2 + (1 if act == 'lrelu' else 0)
    _judge('fwd %s %s' % (name, kind), out.cpu().double(), x, wt, bias, res, act, slope, exact_class, K, e)


@pytest.mark.parametrize('co', [64, 128])
def test_bf16_operands_give_the_one_term_kernels_result(pkg, dev, co):
    """The two-term kernel is the one-term kernel plus two sweeps of small terms.  With every operand a bf16 value, split2's second
    term x - bf16(x) is exactly zero, the sweeps x1 w2 and x2 w1 add zeros, and the one-term and two-term kernels return EQUAL
    values (compared as floats: an accumulator of -0 may come back +0).  No reference is involved.  One image of 9 x 33 pixels
    (a tile edge crossed both ways), two 32-channel chunks through the concat, bias + residual + LeakyReLU in the shared epilogue,
    BN = 64 and BN = 128."""
    n, c1, c2, h, w = 1, 32, 32, 9, 33
    K = 9 * (c1 + c2)
    g = _g(450 + co)
    x, wt = R.rb(R.normal((n, c1 + c2, h, w), g)), R.rb(R.normal((co, c1 + c2, 3, 3), g, K ** -0.5))
    bias, res = R.normal((co,), g), R.normal((n, co, h, w), g)
    xs1 = LP.poisoned_slice(x[:, :c1].contiguous(), c1 + 32, 16, dev)
    xs2 = LP.poisoned_slice(x[:, c1:].contiguous(), c2 + 16, 8, dev)
    rs = LP.poisoned_slice(res, co + 16, 8, dev)
    got = {}
    for family, ids in (('bf16x1', (70, 71)), ('bf16x2', (90, 91))):
        out = LP.canary_slice(n, co, h, w, co + 8, 4, dev)
        kid = _launch_fwd(pkg, xs1, xs2, wt.to(dev), bias.to(dev), rs, out, 2, 0.25, family)
        assert kid == ids[0 if co % 128 == 0 else 1]
        for t in (xs1, xs2, rs):
            LP.check_slice(t)
        LP.check_slice(out, written=True)
        got[family] = out.cpu()
    assert bool(torch.isfinite(got['bf16x1']).all().item()) and bool((got['bf16x1'] < 0).any().item())
    assert torch.equal(got['bf16x1'], got['bf16x2'])


@pytest.mark.parametrize('kind', ['ints', 'x12', 'w12', 'normal'])
@pytest.mark.parametrize('name', sorted(R.DGRAD_CASES))
def test_input_gradient_channel_window(pkg, dev, name, kind):
    ops = pkg.ops
    n, o, i, c_lo, c_hi, h, w = R.DGRAD_CASES[name]
    rows, K = c_hi - c_lo, 9 * o
    g = _g(200 + len(name) + len(kind))
    dy, wt, exact_class = _data(kind, (n, o, h, w), (o, i, 3, 3), g, K)
    res = R.small_ints((n, rows, h, w), g) if exact_class else R.normal((n, rows, h, w), g)
    dys = LP.poisoned_slice(dy, o + 32, 16, dev)
    rs = LP.poisoned_slice(res, rows + 16, 8, dev)
    out = LP.canary_slice(n, rows, h, w, rows + 8, 4, dev)
    kid = _launch_dgrad(pkg, dys, wt.to(dev), c_lo, c_hi, rs, out)
    assert kid == (90 if rows % 128 == 0 else 91)
    LP.check_slice(dys); LP.check_slice(rs); LP.check_slice(out, written=True)
    _judge('dgrad %s %s' % (name, kind), out.cpu().double(), dy, R.dgrad_weight(wt, c_lo, c_hi), None, res, None, 0.0, exact_class, K, 1)


@pytest.mark.parametrize('side', ['x', 'w'])
@pytest.mark.parametrize('value', [float('inf'), float('nan'), 3.39e38], ids=['inf', 'nan', '3.39e38'])
def test_nonfinite_operands_give_the_fp32_kernels_pattern(pkg, dev, side, value):
    ops = pkg.ops
    n, c1, c2, co, h, w, act, code, slope = R.FWD_CASES['k1_c64_9x33']
    K = 9 * c1
    g = _g(300)
    x, wt = R.normal((n, c1, h, w), g), R.normal((co, c1, 3, 3), g, K ** -0.5)
    clean_x, clean_w = x.clone(), wt.clone()
    if side == 'x':
        x[1, 7, 4, 20] = value
    else:
        wt[33, 5, 1, 2] = value
    xd, wd = ops.to_nhwc(x.to(dev)), wt.to(dev)
    out = ops.new_nhwc(n, co, h, w, dev)
    assert _launch_fwd(pkg, xd, None, wd, None, None, out, 0, 0.0) == 91
    y = out.cpu().double()
    y32 = ops._conv_fwd_impl(xd, None, wd, None, 1, 1, 0, 0.0).cpu().double()
    for pred in (torch.isnan, torch.isposinf, torch.isneginf):
        assert torch.equal(pred(y), pred(y32)), pred.__name__
    fin = torch.isfinite(y32)
    if value == 3.39e38 and side == 'x':
        assert fin.all()                           # finite in fp32 (|w| < 1): the guard's own case (bf16 infinity, then a NaN second term)
    elif value != 3.39e38:
        assert 0 < (~fin).sum().item() < fin.numel()
    # the finite values: class (3)'s gate around the exact result, the a-priori terms from the operands as given (finite ones)
    xf, wf = (clean_x if side == 'x' else x), (clean_w if side == 'w' else wt)
    if value == 3.39e38:
        xf, wf = x, wt
    with np.errstate(all='ignore'):
        exact = R.conv_exact(x, wt)
    mag = R.conv_mag(xf, wf)
    gate = R.conv_acc_gate(K, mag, exact.nan_to_num(0.0, 0.0, 0.0)) + R.BOUND * mag
    assert ((y - exact).abs()[fin] <= gate[fin]).all()


def test_pack_bytes_match_the_restatement(pkg, dev):
    ops, lib = pkg.ops, pkg._lib
    g = _g(400)
    for co, cin in ((128, 64), (192, 32)):
        wt = R.normal((co, cin, 3, 3), g).to(dev)
        wpk, kp, kmode = ops._pack(wt, 0, ops._X1_TAPS, cin, cin)
        assert kmode == 0 and kp == 9 * cin
        fmt = 2128 if co % 128 == 0 else 2064
        nbytes = lib.call('ssg_pack_weights_bf16x2_bytes', co, kp, fmt)
        assert nbytes == co * kp * 4
        buf = torch.zeros(nbytes // 2, dtype=torch.int16, device=dev)
        lib.call('ssg_pack_weights_bf16x2', wpk.data_ptr(), co, kp, fmt, ops.ptr(buf), ops.stream_ptr())
        want = R.pack_x2(wpk.cpu().numpy().reshape(-1)[:co * kp].reshape(co, kp), fmt - 2000)
        got = buf.cpu().numpy().view(np.uint16).reshape(want.shape)
        assert np.array_equal(got, want)
    for bad in ((128, 288, 1128), (96, 288, 2128), (128, 144, 2128), (128, 288, 64)):
        assert lib.call('ssg_pack_weights_bf16x2_bytes', *bad) == 0


def test_refusals_launch_nothing(pkg, dev):
    ops, lib = pkg.ops, pkg._lib
    mk = lambda *s: torch.randn(*s, device=dev)

    def refused(d, out):
        assert lib.call('ssg_conv2d_bf16x2_ok', C.byref(d)) == 0
        assert lib.call('ssg_conv2d_bf16x2_kernel_id', C.byref(d)) < 0
        assert lib.load().ssg_conv2d_bf16x2_f32(C.byref(d), C.c_void_p(16), None) != 0
        assert b'bf16x2' in lib.load().ssg_last_error()
        torch.cuda.synchronize()
        assert bool(LP.is_canary(out).all().item()), 'a refused call wrote the output'

    ops.PROFILE = []
    try:
        x, w = ops.to_nhwc(mk(1, 64, 20, 20)), mk(64, 64, 3, 3)

        def desc(x=x, w=w):
            out = LP.canary_fill_(ops.new_nhwc(x.shape[0], w.shape[0], x.shape[2], x.shape[3], dev))
            d = ops._x1_desc(x, None, w, None, out)
            wpk, kp, kmode = ops._pack(w, 0, ops._X1_TAPS, w.shape[1], x.shape[1])
            d.w = wpk.data_ptr(); d.Kp = kp; d.kmode = kmode
            return d, out, wpk
        d, out, keep = desc()
        assert lib.call('ssg_conv2d_bf16x2_ok', C.byref(d)) == 2064                    # the legal descriptor the refusals start from
        d.dx[4] = 2                                                                     # a wrong tap set
        refused(d, out)
        d, out, keep = desc()
        d.in_sy = d.in_sx = 2; d.GH = d.GW = d.OH = d.OW = 10                           # stride 2
        refused(d, out)
        d, out, keep = desc(x=ops.to_nhwc(mk(1, 64, 20, 16)))                           # 16 pixels wide
        refused(d, out)
        d, out, keep = desc(w=mk(96, 64, 3, 3))                                         # Cout not a multiple of 64
        refused(d, out)
        assert not ops.conv2d_bf16x2_ok(mk(1, 64, 20, 16), mk(64, 64, 3, 3))
        assert ops.PROFILE == []
    finally:
        ops.PROFILE = None
