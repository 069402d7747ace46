"""csrc/depthwise.hip against tests/dw_ref.py: the depthwise convolution (forward, input gradient, weight gradient, every generic
and register-tiled kernel), channel scale / per-sample channel sum / row broadcast, and the unary ops and the product, fp32 and
bf16, entry point by entry point through the C-ABI (ld > C, offset slices, a scale on the channel sum) and assembled through
ops.* / bf16.*.  tests/test_dw_ref.py rehearses every gate used here on the CPU: an emulation of each tiled kernel passes it at
these very cases, and each planted defect fails it.

Every gate is a rounding count times a unit roundoff times a magnitude sum of the fp64 reference plus one output rounding; the
counts are derived in dw_ref.py beside each gate.  No case is filtered by value.  Every output is pre-filled with NaN (an
element left unwritten fails), sliced outputs have their neighbouring channels checked for writes, workspaces are used at
exactly the queried size with a guard band behind, and the weight gradients and channel sums run twice and must give the same
bits.  Each convolution case asserts the kernel id ssg_dwconv2d_kernel_id names for the pointers it actually passes, so the
table's coverage (dw_ref.check_coverage: every id x op x dtype) is coverage of what ran.

No defect was found in depthwise.hip: every case passes on every route.  (What the old tests could not have seen -- a dropped
last column where OW % 4 != 0, a wrong tap on one pad parity, a lost last x-quad or part of the weight gradient, a truncating
bf16 store -- each fails here; tests/test_dw_ref.py shows it on the emulations.)

Worst measured error / gate per family on an MI355X (pass: <= 1; the CPU rehearsal's emulation figure in brackets, tiled routes only):

    forward fp32                0.35 generic, 0.33 tiled S=1, 0.23 tiled S=2                       [0.34, 0.28]
    forward bf16                0.996 generic, 0.995 tiled S=1, 0.984 tiled S=2                    [0.995, 0.984]
    input gradient fp32         0.38 generic, 0.34 flipped S=1, 0.17 / 0.18 S=2 PLODD 0 / 1        [0.33, 0.22, 0.18]
    input gradient bf16         0.996 generic, 0.996 flipped S=1, 0.996 / 0.995 S=2 PLODD 0 / 1    [0.996, 0.996, 0.995]
    weight gradient fp32        0.987 generic, 0.983 tiled S=1, 0.991 tiled S=2                    [0.983, 0.991]
    weight gradient bf16        0.22 generic, 0.19 tiled S=1, 0.16 tiled S=2                       [0.19, 0.16]
    channel sum                 fp32 0.996 (a), 0.75 (a b); bf16 0.018, 0.020                      [0.998, 0.75; 0.018, 0.020]
    channel scale / broadcast   fp32 0.998 / 0.999; bf16 0.988 / 0.981
    unary y, dx                 swish 0.51, 0.44; sigmoid 0.49, 0.48; gaussian 0.91, 0.88          [0.51, 0.40; 0.50, 0.48; 0.91, 0.88]
    product                     0.99 y, 0.98 da, 0.995 db
    ops.dwconv2d / bf16.dwconv2d   fp32 0.20 y, 0.22 dx, 0.87 dw; bf16 0.99 y, 0.99 dx, 0.05 dw
    channel_scale / global_avgpool fp32 0.998 y, 0.998 dx, 0.47 ds, 0.89 pool, 0.79 pool dx; bf16 0.98, 0.98, 0.02, 0.03, 0.62
    two runs of every weight gradient and channel sum: the same bits

  (the fp32 weight gradient and channel sum, scale, broadcast, product and the bf16 stores are single roundings of an accurately
  known value: a half-ulp bound is met close to 1.  The bf16 reductions sit far below their gate, which charges every fp32
  addition of a thread's chain its worst case.)

In one run on an MI355X the file's 266 cases take 9 s; the two 16 x 1024 x 2688 channel sums (the shape at which 2048 / blocks
limits the slice count, 176 MB in fp32) take 1.9 s each, most of it the host's data and fp64 reference, every other case under 0.2 s
after the first launch.
"""
import ctypes as C_

import numpy as np
import pytest
import torch

import dw_ref as dr
from dw_ref import F32, F64, OP_DGRAD, OP_FWD, OP_WGRAD, f32

pytestmark = pytest.mark.gpu

GUARD = 512
POISON = 0xA5
BF = torch.bfloat16
NAN = float('nan')


def _report(family, ratios):
    print('RATIO %-28s %s' % (family, '  '.join('%s=%.3g' % kv for kv in sorted(ratios.items()))))


def _ok(ratios):
    return all(v <= 1.0 for v in ratios.values())


def _np(t):
    t = t.detach()
    return np.ascontiguousarray((t.float() if t.dtype == BF else t).cpu().numpy())


def _sfx(bf16):
    return '_bf16' if bf16 else '_f32'


def _dt(bf16):
    return 'bf16' if bf16 else 'f32'


class _Ws(object):
    """A workspace of exactly `nbytes`, NaN-filled, with a poisoned guard band behind it that must survive."""

    def __init__(self, nbytes, dev):
        self.n = int(nbytes)
        assert self.n % 8 == 0
        self.buf = torch.empty(self.n + GUARD, dtype=torch.uint8, device=dev)
        assert self.buf.data_ptr() % 16 == 0
        self.fill()

    def fill(self):
        self.buf[:self.n].view(torch.float64).fill_(NAN)
        self.buf[self.n:] = POISON

    def ptr(self):
        return C_.c_void_p(self.buf.data_ptr())

    def intact(self):
        return bool((self.buf[self.n:] == POISON).all().item())


class _Rows(object):
    """`rows` x C values as the channel slice [off, off + C) of NaN-filled rows `ld` wide (ld = C, off = 0: dense)."""

    def __init__(self, dev, rows, C, ld, off, bf16, data=None):
        assert off + C <= ld
        self.C, self.ld, self.off, self.bf16 = C, ld, off, bf16
        self.buf = torch.full((rows, ld), NAN, dtype=BF if bf16 else torch.float32, device=dev)
        if data is not None:
            t = torch.from_numpy(np.array(f32(data).reshape(rows, C), order='C')).to(dev)         # a copy: cached data is read-only
            self.buf[:, off:off + C] = t.to(BF) if bf16 else t

    def ptr(self):
        return C_.c_void_p(self.buf.data_ptr() + self.off * self.buf.element_size())

    def aligned16(self):
        return (self.buf.data_ptr() + self.off * self.buf.element_size()) % 16 == 0

    def values(self, shape):
        return _np(self.buf[:, self.off:self.off + self.C]).reshape(shape)

    def neighbours_untouched(self):
        b = self.buf
        return bool(torch.isnan(b[:, :self.off].float()).all().item() and torch.isnan(b[:, self.off + self.C:].float()).all().item())


class _Abi(object):
    """The C-ABI entry points of depthwise.hip, pointers, strides and the stream filled in."""

    def __init__(self, pkg, dev):
        self.lib, self.dev = pkg._lib, dev

    def call(self, name, *a):
        return self.lib.call(name, *(a + (self.lib.stream_ptr(),)))

    def dev_f32(self, a):
        return torch.from_numpy(np.ascontiguousarray(f32(a))).to(self.dev)

    def rows(self, rows, C, ld, off, bf16, data=None):
        return _Rows(self.dev, rows, C, ld, off, bf16, data)


@pytest.fixture()
def abi(pkg, dev):
    return _Abi(pkg, dev)


def _bits_equal(a, b):
    return dr.same_bits(a, b)


# ----------------------------------------------------------------------------- 1. depthwise convolution, every route
@pytest.mark.parametrize('bf16,case', [(b, c) for b in (False, True) for c in dr.dw_cases(b)],
                         ids=lambda v: v.name if isinstance(v, tuple) else _dt(v))
def test_dwconv(abi, bf16, case):
    c = case
    lib = abi.lib
    N, H, W, C, KH, KW, s = c.N, c.H, c.W, c.C, c.KH, c.KW, c.stride
    pt, _, pl, _ = c.pads
    OH, OW = dr.out_hw(H, W, KH, KW, s, c.pads)
    ldx, ldy, lddy, lddx = c.lds or (C, C, C, C)
    off = c.off[1 if bf16 else 0]
    x, w, b, g = dr.dw_data(c, bf16)
    wd, bd = abi.dev_f32(w), abi.dev_f32(b)
    xr = abi.rows(N * H * W, C, ldx, off, bf16, x)
    gr = abi.rows(N * OH * OW, C, lddy, off, bf16, g)
    sfx = _sfx(bf16)
    taps = KH * KW
    ratios = {}
    if 'f' in c.ops:
        yr = abi.rows(N * OH * OW, C, ldy, off, bf16)
        rid = lib.call('ssg_dwconv2d_kernel_id', OP_FWD, s, KH, KW, pl, N * OH, C, int(xr.aligned16() and yr.aligned16()))
        assert rid == dr.case_route(c, OP_FWD, bf16), 'forward ran kernel id %d' % rid
        abi.call('ssg_dwconv2d_fwd' + sfx, xr.ptr(), N, H, W, C, ldx, lib.ptr(wd), lib.ptr(bd), KH, KW, s, pt, pl, OH, OW, yr.ptr(), ldy)
        ref, mag = dr.fwd_ref(x, w, b, s, c.pads)
        ratios['fwd%d' % rid] = dr.conv_ratio(yr.values(ref.shape), ref, mag, taps, bf16)
        assert yr.neighbours_untouched(), 'forward wrote outside its channel slice'
    if 'd' in c.ops:
        dxr = abi.rows(N * H * W, C, lddx, off, bf16)
        rid = lib.call('ssg_dwconv2d_kernel_id', OP_DGRAD, s, KH, KW, pl, N * H, C, int(gr.aligned16() and dxr.aligned16()))
        assert rid == dr.case_route(c, OP_DGRAD, bf16), 'input gradient ran kernel id %d' % rid
        abi.call('ssg_dwconv2d_dgrad' + sfx, gr.ptr(), lddy, N, H, W, C, lib.ptr(wd), KH, KW, s, pt, pl, OH, OW, dxr.ptr(), lddx)
        ref, mag = dr.dgrad_ref(g, w, s, c.pads, H, W)
        ratios['dgrad%d' % rid] = dr.conv_ratio(dxr.values(ref.shape), ref, mag, taps, bf16)
        assert dxr.neighbours_untouched(), 'input gradient wrote outside its channel slice'
    if 'w' in c.ops:
        rid = lib.call('ssg_dwconv2d_kernel_id', OP_WGRAD, s, KH, KW, pl, 0, C, 1)
        assert rid == dr.case_route(c, OP_WGRAD, bf16)
        ws = _Ws(lib.call('ssg_dwconv2d_wgrad_workspace_bytes', N, OH, OW, C, KH, KW), abi.dev)
        runs = []
        for _ in range(2):                               # twice: ordered second stage, no atomics -> the same bits
            ws.fill()
            dw = torch.full((C, KH, KW), NAN, dtype=torch.float32, device=abi.dev)
            abi.call('ssg_dwconv2d_wgrad' + sfx, xr.ptr(), N, H, W, C, ldx, gr.ptr(), lddy, KH, KW, s, pt, pl, OH, OW, lib.ptr(dw), ws.ptr())
            runs.append(_np(dw))
        assert ws.intact(), 'guard band behind the weight-gradient workspace'
        assert _bits_equal(runs[0], runs[1]), 'two weight-gradient runs differ'
        ref, mag = dr.wgrad_ref(x, g, KH, KW, s, c.pads)
        ratios['wgrad%d' % rid] = dr.wgrad_ratio(runs[0], ref, mag, c, bf16)
    _report('dwconv %s %s' % (_dt(bf16), c.name), ratios)
    assert _ok(ratios), ratios


# ----------------------------------------------------------------------------- 2. per-sample channel sum
def _channel_sum(abi, bf16, N, S, C, lda, ldb, a, b):
    lib = abi.lib
    ar = abi.rows(N * S, C, lda, (lda - C) // 2 // 8 * 8, bf16, a)
    br_ = abi.rows(N * S, C, ldb, (ldb - C) // 8 * 8, bf16, b)
    ws = _Ws(lib.call('ssg_sample_channel_sum_workspace_bytes', N, S, C), abi.dev)
    ratios = {}
    for name, bb, scale in (('a', None, 1.0 / S), ('ab', br_, 0.75)):
        runs = []
        for _ in range(2):
            ws.fill()
            out = torch.full((N, C), NAN, dtype=torch.float32, device=abi.dev)
            abi.call('ssg_sample_channel_sum' + _sfx(bf16), ar.ptr(), lda, bb.ptr() if bb is not None else None, ldb if bb is not None else 0,
                     N, S, C, scale, lib.ptr(out), ws.ptr())
            runs.append(_np(out))
        assert ws.intact(), 'guard band behind the channel-sum workspace'
        assert _bits_equal(runs[0], runs[1]), 'two channel-sum runs differ'
        ref, mag = dr.channel_sum_ref(a, b if bb is not None else None, scale)
        ratios[name] = dr.colsum_ratio(runs[0], ref, mag, N, S, C, bf16, bb is not None)
    return ratios


@pytest.mark.parametrize('bf16', [False, True], ids=['f32', 'bf16'])
@pytest.mark.parametrize('case', dr.COLSUM_CASES, ids=lambda c: '%dx%dx%d' % c)
def test_sample_channel_sum(abi, bf16, case):
    N, S, C = case
    a, b = dr.colsum_data(N, S, C, bf16)
    ratios = _channel_sum(abi, bf16, N, S, C, C, C, a, b)
    _report('channel sum %s %dx%dx%d' % ((_dt(bf16),) + case), ratios)
    assert _ok(ratios), ratios


@pytest.mark.parametrize('bf16', [False, True], ids=['f32', 'bf16'])
def test_sample_channel_sum_of_slices(abi, bf16):
    N, S, C, lda, ldb = dr.COLSUM_LD
    a, b = dr.colsum_data(N, S, C, bf16)
    ratios = _channel_sum(abi, bf16, N, S, C, lda, ldb, a, b)
    _report('channel sum %s slices' % _dt(bf16), ratios)
    assert _ok(ratios), ratios


# ----------------------------------------------------------------------------- 3. channel scale, row broadcast
@pytest.mark.parametrize('bf16', [False, True], ids=['f32', 'bf16'])
@pytest.mark.parametrize('case', dr.SE_CASES, ids=lambda c: '%dx%dx%d' % c)
def test_channel_scale_and_broadcast(abi, bf16, case):
    N, S, C = case
    lib = abi.lib
    x, s = dr.se_data(N, S, C, bf16)
    sd = abi.dev_f32(s)
    ratios = {}
    for tag, ldx, ldy, off in (('dense', C, C, 0), ('slice', C + 16, C + 8, 8)):
        xr = abi.rows(N * S, C, ldx, off, bf16, x)
        yr = abi.rows(N * S, C, ldy, off, bf16)
        abi.call('ssg_channel_scale_fwd' + _sfx(bf16), xr.ptr(), ldx, lib.ptr(sd), N, S, C, yr.ptr(), ldy)
        ref = dr.channel_scale_ref(x, s)
        ratios['scale_' + tag] = dr.worst_ratio(yr.values(ref.shape) - ref, dr.one_rounding_gate(ref, bf16))
        assert yr.neighbours_untouched()
        for scale in (0.75, 1.0 / 256):                  # bf16-representable, so the bf16 store is the one rounding
            yr = abi.rows(N * S, C, ldy, off, bf16)
            abi.call('ssg_broadcast_rows' + _sfx(bf16), lib.ptr(sd), N, S, C, scale, yr.ptr(), ldy)
            ref = dr.broadcast_ref(s, scale, S)
            ratios['bcast_%s_%g' % (tag, scale)] = dr.worst_ratio(yr.values(ref.shape) - ref, dr.one_rounding_gate(ref, bf16))
            assert yr.neighbours_untouched()
    _report('scale / broadcast %s %dx%dx%d' % ((_dt(bf16),) + case), ratios)
    assert _ok(ratios), ratios


# ----------------------------------------------------------------------------- 4. unary ops and the product (fp32)
@pytest.mark.parametrize('op', [dr.UNARY_SWISH, dr.UNARY_SIGMOID, dr.UNARY_GAUSSIAN], ids=['swish', 'sigmoid', 'gaussian'])
@pytest.mark.parametrize('case', dr.UNARY_CASES, ids=lambda c: '%dx%d_ld%d_%d' % c)
def test_unary(abi, op, case):
    P, C, ldx, ldy = case
    z, g = dr.unary_data(P, C)
    assert z.size >= len(dr.Z_SWEEP)
    offx, offy = (ldx - C) // 8 * 4, (ldy - C) // 4 * 4
    zr = abi.rows(P, C, ldx, offx, False, z)
    gr = abi.rows(P, C, ldx, offx, False, g)
    yr = abi.rows(P, C, ldy, offy, False)
    dxr = abi.rows(P, C, ldy, offy, False)
    abi.call('ssg_unary_fwd_f32', zr.ptr(), ldx, P, C, op, yr.ptr(), ldy)
    abi.call('ssg_unary_bwd_f32', zr.ptr(), ldx, gr.ptr(), ldx, P, C, op, dxr.ptr(), ldy)
    y_ref, d_ref = dr.unary_ref(z, op)
    gy, gd = dr.unary_gates(z, op, g)
    with np.errstate(all='ignore'):
        ratios = dict(y=dr.unary_ratio(yr.values(z.shape), y_ref, gy), dx=dr.unary_ratio(dxr.values(z.shape), g.astype(F64) * d_ref, gd))
    assert yr.neighbours_untouched() and dxr.neighbours_untouched()
    _report('unary op %d %dx%d' % (op, P, C), ratios)
    assert _ok(ratios), ratios


@pytest.mark.parametrize('op', [dr.UNARY_SWISH, dr.UNARY_SIGMOID, dr.UNARY_GAUSSIAN], ids=['swish', 'sigmoid', 'gaussian'])
def test_unary_forward_zeroes_the_pad_lanes(abi, op):
    P, C, ldx, ldy = dr.UNARY_PAD_CASE
    z, _ = dr.unary_data(P, C)
    buf = np.zeros((P, ldx), dtype=F32); buf[:, :C] = z
    zd = abi.dev_f32(buf)
    yd = torch.full((P, ldy), NAN, dtype=torch.float32, device=abi.dev)
    abi.call('ssg_unary_fwd_f32', abi.lib.ptr(zd), ldx, P, C, op, abi.lib.ptr(yd), ldy)
    y = _np(yd)
    y_ref, _ = dr.unary_ref(z, op)
    gy, _ = dr.unary_gates(z, op)
    with np.errstate(all='ignore'):
        r = dr.unary_ratio(y[:, :C], y_ref, gy)
    assert r <= 1.0, r
    assert np.array_equal(y[:, C:(C + 3) // 4 * 4].view(np.int32), np.zeros((P, (C + 3) // 4 * 4 - C), dtype=np.int32)), 'pad lanes must be +0'


@pytest.mark.parametrize('case', dr.UNARY_CASES, ids=lambda c: '%dx%d_ld%d_%d' % c)
def test_mul(abi, case):
    P, C, ldx, ldy = case
    a, g = dr.unary_data(P, C)
    a = np.nan_to_num(a, nan=1.5, posinf=3e38, neginf=-3e38)      # the sweep's finite extremes stay: 1e-30 * 1e4, 3e38 * 0.x
    b = f32(dr.unary_data(P, C, seed=29)[1])
    ar = abi.rows(P, C, ldx, 0, False, a); br_ = abi.rows(P, C, ldy, 0, False, b); gr = abi.rows(P, C, ldx + 8, 4, False, g)
    yr = abi.rows(P, C, ldy + 8, 4, False); dar = abi.rows(P, C, ldx + 16, 8, False); dbr = abi.rows(P, C, ldy + 24, 4, False)
    abi.call('ssg_mul_fwd_f32', ar.ptr(), ldx, br_.ptr(), ldy, P, C, yr.ptr(), ldy + 8)
    abi.call('ssg_mul_bwd_f32', ar.ptr(), ldx, br_.ptr(), ldy, gr.ptr(), ldx + 8, P, C, dar.ptr(), ldx + 16, dbr.ptr(), ldy + 24)
    a64, b64, g64 = a.astype(F64), b.astype(F64), g.astype(F64)
    ratios = {}
    with np.errstate(all='ignore'):
        for name, rows, ref in (('y', yr, a64 * b64), ('da', dar, g64 * b64), ('db', dbr, g64 * a64)):
            ref = np.where(np.abs(ref) > 3.4028234663852886e38, np.sign(ref) * np.inf, ref)          # fp32 overflow is the product's class
            ratios[name] = dr.unary_ratio(rows.values(a.shape), ref, dr.one_rounding_gate(np.nan_to_num(ref, posinf=0, neginf=0)) + dr.MIN_NORMAL)
            assert rows.neighbours_untouched()
    _report('mul %dx%d' % (P, C), ratios)
    assert _ok(ratios), ratios


# ----------------------------------------------------------------------------- 5. assembled: the public ops of both packages
def _nchw(a, dev, bf16=False, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(f32(a).transpose(0, 3, 1, 2))).to(dev)
    if bf16:
        t = t.to(BF).contiguous(memory_format=torch.channels_last)
    return t.requires_grad_(True) if grad else t


def _nhwc(t):
    return np.ascontiguousarray(_np(t).transpose(0, 2, 3, 1))


PUBLIC_DW = ['c64_s1k3', 'c68_s2k5', 's1k9_same', 's2k3_7x10_p0101', 's2k5_8x9_p1212', 'rect3x5_s2', 'k4', 'w67_s2k5']


@pytest.mark.parametrize('bf16', [False, True], ids=['f32', 'bf16'])
@pytest.mark.parametrize('name', PUBLIC_DW)
def test_public_dwconv2d(pkg, dev, bf16, name):
    c = next(k for k in dr.DW_CASES if k.name == name)
    if bf16 and c.C % 8:                                 # bf16 tensors of the package are dense with C % 8 == 0: the same case at C + 4
        c = c._replace(C=c.C + 4)
    x, w, b, g = dr.dw_data(c, bf16)
    xt = _nchw(x, dev, bf16, grad=True)
    wt = torch.from_numpy(np.ascontiguousarray(w[:, None])).to(dev).requires_grad_(True)
    if bf16:
        b = None
        y = pkg.bf16.dwconv2d(xt, wt, stride=c.stride, padding=c.pads)
    else:
        y = pkg.ops.dwconv2d(xt, wt, torch.from_numpy(b).to(dev), stride=c.stride, padding=c.pads)
    y.backward(_nchw(g, dev, bf16))
    taps = c.KH * c.KW
    ref, mag = dr.fwd_ref(x, w, b, c.stride, c.pads)
    dref, dmag = dr.dgrad_ref(g, w, c.stride, c.pads, c.H, c.W)
    wref, wmag = dr.wgrad_ref(x, g, c.KH, c.KW, c.stride, c.pads)
    ratios = dict(y=dr.conv_ratio(_nhwc(y), ref, mag, taps, bf16), dx=dr.conv_ratio(_nhwc(xt.grad), dref, dmag, taps, bf16),
                  dw=dr.wgrad_ratio(_np(wt.grad)[:, 0], wref, wmag, c, bf16))
    _report('public dwconv2d %s %s' % (_dt(bf16), name), ratios)
    assert _ok(ratios), ratios


@pytest.mark.parametrize('bf16', [False, True], ids=['f32', 'bf16'])
@pytest.mark.parametrize('shape', [(2, 16, 16, 8), (3, 1, 1, 136), (2, 64, 65, 8)], ids=lambda s: '%dx%dx%dx%d' % s)
def test_public_squeeze_excite(pkg, dev, bf16, shape):
    N, H, W, C = shape
    S = H * W
    m = pkg.bf16 if bf16 else pkg.ops
    x, s = dr.se_data(N, S, C, bf16)
    g, _ = dr.se_data(N, S, C, bf16, seed=31)
    xt = _nchw(x.reshape(N, H, W, C), dev, bf16, grad=True)
    st = torch.from_numpy(s).to(dev).view(N, C, 1, 1).requires_grad_(True)
    y = m.channel_scale(xt, st)
    y.backward(_nchw(g.reshape(N, H, W, C), dev, bf16))
    ref = dr.channel_scale_ref(x, s)
    geo = dr.colsum_geom(N, S, C)
    ds_ref, ds_mag = dr.channel_sum_ref(g, x, 1.0)
    ratios = dict(y=dr.worst_ratio(_nhwc(y).reshape(N, S, C) - ref, dr.one_rounding_gate(ref, bf16)),
                  dx=dr.worst_ratio(_nhwc(xt.grad).reshape(N, S, C) - dr.channel_scale_ref(g, s), dr.one_rounding_gate(dr.channel_scale_ref(g, s), bf16)),
                  ds=dr.worst_ratio(_np(st.grad).reshape(N, C) - ds_ref, dr.channel_sum_gate(ds_ref, ds_mag, S, geo.chain, bf16, True)))
    xp = _nchw(x.reshape(N, H, W, C), dev, bf16, grad=True)
    pooled = m.global_avgpool(xp)
    pg = dr.se_data(N, 1, C, True, seed=37)[0].reshape(N, C)         # bf16-representable pooled gradient
    pooled.backward(torch.from_numpy(pg).to(dev).view(N, C, 1, 1))
    p_ref, p_mag = dr.channel_sum_ref(x, None, 1.0 / S)
    ratios['pool'] = dr.worst_ratio(_np(pooled).reshape(N, C) - p_ref, dr.channel_sum_gate(p_ref, p_mag, S, geo.chain, bf16, False))
    b_ref = dr.broadcast_ref(pg, 1.0 / S, S)
    if not bf16 or (S & (S - 1)) == 0:                   # bf16: one rounding only where 1 / S is a power of two
        ratios['pool_dx'] = dr.worst_ratio(_nhwc(xp.grad).reshape(N, S, C) - b_ref, dr.one_rounding_gate(b_ref, bf16))
    else:                                                # else the fp32 product rounds before the store does
        ratios['pool_dx'] = dr.worst_ratio(_nhwc(xp.grad).reshape(N, S, C) - b_ref, dr.one_rounding_gate(b_ref, True) + dr.one_rounding_gate(b_ref, False))
    _report('public squeeze-excite %s %dx%dx%dx%d' % ((_dt(bf16),) + shape), ratios)
    assert _ok(ratios), ratios


@pytest.mark.parametrize('op', [dr.UNARY_SWISH, dr.UNARY_SIGMOID, dr.UNARY_GAUSSIAN], ids=['swish', 'sigmoid', 'gaussian'])
def test_public_unary_and_mul(pkg, dev, op):
    N, H, W, C = 2, 5, 7, 12
    z, g = dr.unary_data(N * H * W, C)
    fn = (pkg.ops.swish, pkg.ops.sigmoid, pkg.ops.gaussian)[op]
    zt = _nchw(z.reshape(N, H, W, C), dev, grad=True)
    y = fn(zt)
    y.backward(_nchw(g.reshape(N, H, W, C), dev))
    y_ref, d_ref = dr.unary_ref(z, op)
    gy, gd = dr.unary_gates(z, op, g)
    with np.errstate(all='ignore'):
        ratios = dict(y=dr.unary_ratio(_nhwc(y).reshape(z.shape), y_ref, gy), dx=dr.unary_ratio(_nhwc(zt.grad).reshape(z.shape), g.astype(F64) * d_ref, gd))
    a = np.nan_to_num(z, nan=1.5, posinf=2.0, neginf=-2.0)
    at, bt = _nchw(a.reshape(N, H, W, C), dev, grad=True), _nchw(g.reshape(N, H, W, C), dev, grad=True)
    p = pkg.ops.mul(at, bt)
    p.backward(_nchw(np.ones_like(a).reshape(N, H, W, C), dev))
    a64, g64 = a.astype(F64), g.astype(F64)
    ratios['mul'] = dr.worst_ratio(_nhwc(p).reshape(a.shape) - a64 * g64, dr.one_rounding_gate(a64 * g64) + dr.MIN_NORMAL)
    ratios['mul_da'] = 0.0 if dr.same_bits(_nhwc(at.grad).reshape(a.shape), g) else float('inf')
    ratios['mul_db'] = 0.0 if dr.same_bits(_nhwc(bt.grad).reshape(a.shape), a) else float('inf')
    _report('public unary op %d' % op, ratios)
    assert _ok(ratios), ratios
