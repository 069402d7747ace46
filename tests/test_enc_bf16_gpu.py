"""csrc/gemm_bf16.hip, csrc/conv_stem_bf16.hip and the bf16 converts / add of csrc/pointwise.hip against tests/enc_bf16_ref.py,
entry point by entry point through the C-ABI and assembled through bf16.conv1x1 / conv_thin / to_bf16 / to_f32 / add.
tests/test_enc_bf16_ref.py rehearses every gate used here on the CPU: the emulation of each kernel passes it at these very cases
and each planted defect fails it.

Every pixel stride differs from the channel count (ldx = K + 8, ldo = N + 8, ldr = N + 16, ldd = M + 8; stem ldx = 8, ldy = lddy =
Cout + 8, lddx = 8): gaps on inputs hold NaN and are never read, gaps on outputs hold NaN and must survive.  Every output is
pre-filled with NaN, workspaces and dw are used at exactly their size with a poisoned guard band behind, both weight gradients
run twice and must give the same bits, and the three data classes of enc_bf16_ref run at every case of every table: (a) integers,
bit for bit (bf16 outputs: bf16_rne of the exact sum, ties included); (b) one product per output, bit for bit; (c) full-mantissa
random values under the derived per-element gate and the RMS gate against emul() (wgrad_ref.RMS_MARGIN = 2).  The stem forward and
input gradient are fma chains of exact products in a fixed order: their emulations are bit-exact and class (c) compares bits too.

No defect was found in gemm_bf16.hip, conv_stem_bf16.hip or rows_convert_add_kernel: every case passes.  (What the old tests could
not have seen -- a truncating or half-away bf16 store, a dropped K-step or 8-channel tail chunk, a swizzle off by one row group, the
residual read at the output's stride, a wrongly transposed pack, a lost last pixel or last split, stale data in an empty split, swapped
taps, a pad on the wrong side, an unrounded image, a pixel lane wrapping early, a reducer stopping after 64 blocks, a stride parity
ignored -- each fails here; tests/test_enc_bf16_ref.py shows it on the emulations.)

Worst measured error / gate per family on an MI355X (pass: <= 1; an RMS ratio of 0.5 means the kernel's RMS error equals emul()'s):

    pack, both transposes                 bit for bit at all 11 weights, padding +0
    GEMM forward / input gradient         (a), (b): the same bits, res on and off; (c): hard 0.9998 (p127_k24_n120), RMS 0.50 (with res the same)
    GEMM weight gradient                  (a), (b): the same bits at 1 .. 2048 splits; (c): hard 0.26 (p32_8x24), RMS 0.78 (p31_24x8)
    stem forward                          (a), (b): the same bits; (c): the emulation's bits at every case, hard 0.99997 (b2048_k1: a single
                                          product on a tie, half an ulp against half an ulp + 2 u32 |ref|)
    stem weight gradient                  (a), (b): the same bits at 1 .. 2048 blocks; (c): hard 0.17 (ow1_s2), RMS 0.50
    stem input gradient                   (a), (b): the same bits; (c): the emulation's bits at every case, hard 0.32 (b2048_k1)
    converts, add                         bit for bit (ties, +-Inf, NaN, 3.4e38 -> Inf, +-0)
    two runs of both weight gradients     the same bits
    one NaN in x / dy                     exactly its row (GEMM), exactly what its taps reach (stem)

  (a bf16 store is one rounding of an accurately known value: its half-ulp bound is met close to 1.  The fp32 weight gradients sit
  far below their gate, which charges every addition of the chain its worst case; the GEMM weight gradient's RMS error is up to 1.56
  times the emulation's, whose MFMA adds its 16 products and the accumulator with a single rounding.)

In one run on an MI355X the file's 146 cases take 15 s: the 2048-block stem case 1.1 - 2.9 s per class, the 72-block case 2.0 s in
class (c) (the host's emulations), test_conv1x1_autograd 0.8 s (the first launches), every other case under 0.7 s.
"""
import ctypes as C_

import numpy as np
import pytest
import torch

import enc_bf16_ref as er
from enc_bf16_ref import F32, f32
from test_dw_gpu import BF, GUARD, NAN, POISON, _np, _Rows, _Ws

pytestmark = pytest.mark.gpu

GEMM = {c.name: c for c in er.GEMM_CASES}
WG = {c.name: c for c in er.WG_CASES}
STEM = {c.name: c for c in er.STEM_CASES}


class _Out(object):
    """`n` elements of `dtype`, every one NaN, with a poisoned guard band behind them that must survive."""

    def __init__(self, n, dtype, dev):
        self.nbytes = n * torch.empty(0, dtype=dtype).element_size()
        assert self.nbytes % 16 == 0
        self.buf = torch.empty(self.nbytes + GUARD, dtype=torch.uint8, device=dev)
        self.t = self.buf[:self.nbytes].view(dtype)
        self.t.fill_(NAN)
        self.buf[self.nbytes:] = POISON

    def ptr(self):
        return C_.c_void_p(self.buf.data_ptr())

    def intact(self):
        return bool((self.buf[self.nbytes:] == POISON).all().item())


def _report(family, ratios):
    print('RATIO %-34s %s' % (family, '  '.join('%s=%.4g' % kv for kv in sorted(ratios.items()))))


class _Abi(object):
    def __init__(self, pkg, dev):
        self.lib, self.dev = pkg._lib, dev

    def call(self, name, *a):
        return self.lib.call(name, *(a + (self.lib.stream_ptr(),)))

    def f32(self, a):
        return torch.from_numpy(np.ascontiguousarray(f32(a))).to(self.dev)

    def rows(self, rows, C, ld, bf16, data=None):
        return _Rows(self.dev, rows, C, ld, 0, bf16, data)

    def out_f32(self, n):
        """n floats of NaN with a poisoned guard band behind them."""
        return _Out(n, torch.float32, self.dev)

    def pack(self, W, transpose, rows_pad, Kp):
        """ssg_pack_weights_bf16 into NaN-filled storage with a guard band; returns (holder, bf16 view [rows_pad][Kp])."""
        wd = self.f32(W)
        O, I = W.shape
        h = _Out(rows_pad * Kp, BF, self.dev)
        self.call('ssg_pack_weights_bf16', self.lib.ptr(wd), O, I, int(transpose), rows_pad, Kp, h.ptr())
        return h, h.t.view(rows_pad, Kp)


def _floats(out):
    torch.cuda.synchronize()
    return out.t.cpu().numpy().copy()


@pytest.fixture()
def abi(pkg, dev):
    return _Abi(pkg, dev)


def _ids(v):
    return v.name if hasattr(v, 'name') else str(v)


# ----------------------------------------------------------------------------- 1. the pack
@pytest.mark.parametrize('c', er.GEMM_CASES, ids=_ids)
def test_pack_weights(abi, c):
    """Both transposes of every GEMM case's weight, bit for bit with pack_ref, the zero padding of rows and columns included (+0)."""
    _, W, _ = er.gemm_rand_data(c)
    W = f32(W * (1 + 2.0 ** -10))                            # full fp32 mantissas: the pack rounds (ties to even) itself
    W.reshape(-1)[::7] = f32(1 + 2.0 ** -8)                  # ties
    for tr in (0, 1):
        rows, cols = (W.shape[1], W.shape[0]) if tr else W.shape
        rows_pad, Kp = er.round_up(rows, 128), er.round_up(cols, 32) + (32 if 'Kp+32' in c.facts else 0)
        h, wp = abi.pack(W, tr, rows_pad, Kp)
        why = er.first_mismatch(_np(wp), er.pack_ref(W, tr, rows_pad, Kp))
        assert why is None, 'transpose %d: %s' % (tr, why)
        assert h.intact(), 'guard band behind the pack'


# ----------------------------------------------------------------------------- 2. GEMM forward / input gradient
def _gemm_launch(abi, c, x, W, res, poison_rows=True):
    xr = abi.rows(c.P, c.K, c.K + 8, True, x)
    O, I = W.shape
    rows_pad = er.round_up(c.N, 128)
    h, wp = abi.pack(W, c.transpose, rows_pad, c.Kp)
    if c.nan_rows and poison_rows:
        wp[c.N:] = NAN                                       # rows >= N are the zero page's, whatever the pack holds there
    rr = None if res is None else abi.rows(c.P, c.N, c.N + 16, True, res)
    out = abi.rows(c.P, c.N, c.N + 8, True)
    abi.call('ssg_gemm_bf16', xr.ptr(), c.P, c.K, c.K + 8, C_.c_void_p(wp.data_ptr()), c.Kp, c.N, rr.ptr() if rr else None, c.N + 16 if rr else 0,
             out.ptr(), c.N + 8)
    torch.cuda.synchronize()
    assert out.neighbours_untouched(), 'wrote into the gap behind the output channels'
    assert h.intact()
    return out.values((c.P, c.N))


@pytest.mark.parametrize('cls', [0, 1, 2], ids=['int', 'onehot', 'rand'])
@pytest.mark.parametrize('c', er.GEMM_CASES, ids=_ids)
def test_gemm(abi, c, cls):
    ratios = {}
    for variant in ((0, 1) if cls == 1 else (0,)):
        for use_res in ((False,) if cls == 1 else (False, True)):
            x, W, res = er.gemm_data(c, cls, variant)
            res = res if use_res else None
            got = _gemm_launch(abi, c, x, W, res)
            ref, mag = er.gemm_ref(x, er.w_eff(c, W), res, mag=True)
            emu = None
            if cls == 2:
                emu = er.gemm_emul(c, x, er.pack_emul(W, c.transpose, er.round_up(c.N, 128), c.Kp), None if res is None else er.res_buffer(c, res))
            r = er.judge(cls, got, ref, True, er.gemm_gate(c, ref, mag), emu)
            for k, v in r.items():
                ratios['%s%s%s' % (k, '_res' if use_res else '', variant or '')] = v
            if cls < 2:
                assert r['bits'] == 0, er.first_mismatch(got, er.bf16_rne(f32(ref)))
    _report('gemm %s %s' % (('int', 'onehot', 'rand')[cls], c.name), ratios)
    assert er.passes(ratios), ratios


@pytest.mark.parametrize('name', ['p129_k40_n136', 't19_k104_n8', 'p127_k24_n120'])
def test_gemm_one_nan_poisons_exactly_its_row(abi, name):
    """One NaN at x[p][k] makes exactly row p of the output NaN: the tails and the zero page leak nothing."""
    c = GEMM[name]
    x, W, res = er.gemm_rand_data(c)
    for p, k in ((c.P - 1, c.K - 1), (c.P // 2, 0)):
        xn = x.copy(); xn[p, k] = np.nan
        got = _gemm_launch(abi, c, xn, W, res)
        want = np.zeros((c.P, c.N), dtype=bool); want[p] = True
        assert (np.isnan(got) == want).all(), 'NaN at x[%d][%d] reached %d outputs outside row %d' % (p, k, (np.isnan(got) & ~want).sum(), p)


# ----------------------------------------------------------------------------- 3. GEMM weight gradient
def _wg_launch(abi, c, dy, x, runs=2):
    dr = abi.rows(c.P, c.M, c.M + 8, True, dy)
    xr = abi.rows(c.P, c.N, c.N + 16, True, x)
    nbytes = abi.lib.call('ssg_gemm_wgrad_bf16_workspace_bytes', c.P, c.M, c.N)
    assert nbytes == c.ws_bytes and nbytes // (4 * c.M * c.N) == c.splits
    ws = _Ws(nbytes, abi.dev)
    out = []
    for _ in range(runs):
        ws.fill()
        dw = abi.out_f32(c.M * c.N)
        abi.call('ssg_gemm_wgrad_bf16', dr.ptr(), c.M + 8, xr.ptr(), c.N + 16, c.P, c.M, c.N, dw.ptr(), ws.ptr(), nbytes)
        out.append(_floats(dw).reshape(c.M, c.N))
        assert dw.intact(), 'guard band behind dw'
    assert ws.intact(), 'guard band behind the slabs'
    if runs == 2:
        assert er.same_bits(out[0], out[1]), 'two weight-gradient runs differ'
    return out[0]


@pytest.mark.parametrize('cls', [0, 1, 2], ids=['int', 'onehot', 'rand'])
@pytest.mark.parametrize('c', er.WG_CASES, ids=_ids)
def test_gemm_wgrad(abi, c, cls):
    ratios = {}
    for variant in ((0, 1) if cls == 1 else (0,)):
        dy, x = er.wg_data(c, cls, variant)
        got = _wg_launch(abi, c, dy, x)
        ref, mag = er.gemm_wgrad_ref(dy, x, mag=True)
        r = er.judge(cls, got, ref, False, er.wg_gate(c, ref, mag), er.wg_emul(c, dy, x) if cls == 2 else None)
        for k, v in r.items():
            ratios['%s%s' % (k, variant or '')] = v
        if cls < 2:
            assert r['bits'] == 0, er.first_mismatch(got, f32(ref))
    _report('gemm_wgrad %s %s' % (('int', 'onehot', 'rand')[cls], c.name), ratios)
    assert er.passes(ratios), ratios


@pytest.mark.parametrize('name', ['p33_24x24', 'p4133_24x264', 'p16400_24x8'])
def test_gemm_wgrad_one_nan_poisons_exactly_its_row(abi, name):
    c = WG[name]
    dy, x = er.wg_rand_data(c)
    for p, m in ((c.P - 1, c.M - 1), (c.P // 3, 0)):
        dn = dy.copy(); dn[p, m] = np.nan
        got = _wg_launch(abi, c, dn, x, runs=1)
        want = np.zeros((c.M, c.N), dtype=bool); want[m] = True
        assert (np.isnan(got) == want).all(), 'NaN at dy[%d][%d] reached rows other than %d' % (p, m, m)


# ----------------------------------------------------------------------------- 4. the stem
def _x4(c, x):
    x4 = np.zeros((c.N * c.H * c.W, 4), dtype=F32)          # the image's own pad lanes are zero (NHWC contract)
    x4[:, :c.Cin] = f32(x).reshape(-1, c.Cin)
    return x4


def _stem_fwd(abi, c, x, w):
    pt, _, pl, _ = c.pads
    xr = abi.rows(c.N * c.H * c.W, 4, c.ldx, False, _x4(c, x))
    wd = abi.f32(w)
    y = abi.rows(c.N * c.OH * c.OW, c.Cout, c.ldy, True)
    abi.call('ssg_conv2d_thin_bf16', xr.ptr(), c.N, c.H, c.W, c.ldx, abi.lib.ptr(wd), c.Cout, c.Cin, c.KH, c.KW, c.stride, pt, pl, c.OH, c.OW, y.ptr(), c.ldy)
    torch.cuda.synchronize()
    assert y.neighbours_untouched(), 'forward wrote into the gap behind its channels'
    return y.values((c.N, c.OH, c.OW, c.Cout))


def _stem_wgrad(abi, c, x, dy, runs=2):
    pt, _, pl, _ = c.pads
    xr = abi.rows(c.N * c.H * c.W, 4, c.ldx, False, _x4(c, x))
    gr = abi.rows(c.N * c.OH * c.OW, c.Cout, c.ldy, True, dy)
    nbytes = abi.lib.call('ssg_conv2d_thin_bf16_wgrad_workspace_bytes', c.N, c.OH, c.OW, c.Cout, c.KH, c.KW)
    assert nbytes == c.ws_bytes
    ws = _Ws(nbytes, abi.dev)
    out = []
    for _ in range(runs):
        ws.fill()
        dw = abi.out_f32(c.Cout * c.Cin * c.KH * c.KW)
        abi.call('ssg_conv2d_thin_bf16_wgrad', xr.ptr(), c.N, c.H, c.W, c.ldx, gr.ptr(), c.ldy, c.Cout, c.Cin, c.KH, c.KW, c.stride, pt, pl, c.OH, c.OW,
                 dw.ptr(), ws.ptr())
        out.append(_floats(dw).reshape(c.Cout, c.Cin, c.KH, c.KW))
        assert dw.intact(), 'guard band behind dw'
    assert ws.intact(), 'guard band behind the partials'
    if runs == 2:
        assert er.same_bits(out[0], out[1]), 'two stem weight-gradient runs differ'
    return out[0]


def _stem_dgrad(abi, c, dy, w):
    pt, _, pl, _ = c.pads
    gr = abi.rows(c.N * c.OH * c.OW, c.Cout, c.ldy, True, dy)
    wd = abi.f32(w)
    dx = abi.rows(c.N * c.H * c.W, 4, c.ldx, False)
    abi.call('ssg_conv2d_thin_bf16_dgrad', gr.ptr(), c.ldy, c.N, c.H, c.W, abi.lib.ptr(wd), c.Cout, c.Cin, c.KH, c.KW, c.stride, pt, pl, c.OH, c.OW,
             dx.ptr(), c.ldx)
    torch.cuda.synchronize()
    assert dx.neighbours_untouched(), 'input gradient wrote behind its 4-float pixel'
    v = dx.values((c.N, c.H, c.W, 4))
    assert not v[..., c.Cin:].any() and not np.isnan(v[..., c.Cin:]).any(), 'channels Cin .. 3 of the image gradient are not zero'
    return np.ascontiguousarray(v[..., :c.Cin])


def _stem_case(abi, c, cls):
    pt, _, pl, _ = c.pads
    ratios = {}
    for variant in ((0, 1) if cls == 1 else (0,)):
        sfx = str(variant or '')
        x, w, dy = er.stem_data(c, cls, 'fwd', variant)
        got = _stem_fwd(abi, c, x, w)
        ref, mag = er.stem_fwd_ref(x, w, c.stride, pt, pl, c.OH, c.OW, mag=True)
        emu = er.stem_fwd_emul(c, x, w) if cls == 2 else None
        r = er.judge(cls, got, ref, True, er.stem_fwd_gate(c, ref, mag), emu)
        if cls == 2:
            r['emul_bits'] = 0.0 if er.same_bits(got, emu) else float('inf')      # the fma chain of exact products: the same bits
        ratios.update({'fwd_' + k + sfx: v for k, v in r.items()})
        assert er.passes(r), ('fwd', r, er.first_mismatch(got, emu if cls == 2 else er.bf16_rne(f32(ref))))

        x, w, dy = er.stem_data(c, cls, 'wgrad', variant)
        got = _stem_wgrad(abi, c, x, dy)
        ref, mag = er.stem_wgrad_ref(x, dy, c.KH, c.KW, c.stride, pt, pl, mag=True)
        r = er.judge(cls, got, ref, False, er.stem_wgrad_gate(c, ref, mag), er.stem_wgrad_emul(c, x, dy) if cls == 2 else None)
        ratios.update({'wgrad_' + k + sfx: v for k, v in r.items()})
        assert er.passes(r), ('wgrad', r, er.first_mismatch(got, f32(ref)) if cls < 2 else None)

        x, w, dy = er.stem_data(c, cls, 'dgrad', variant)
        got = _stem_dgrad(abi, c, dy, w)
        ref, mag = er.stem_dgrad_ref(dy, w, c.H, c.W, c.stride, pt, pl, mag=True)
        emu = er.stem_dgrad_emul(c, dy, w) if cls == 2 else None
        r = er.judge(cls, got, ref, False, er.stem_dgrad_gate(c, ref, mag), emu)
        if cls == 2:
            r['emul_bits'] = 0.0 if er.same_bits(got, emu) else float('inf')
        ratios.update({'dgrad_' + k + sfx: v for k, v in r.items()})
        assert er.passes(r), ('dgrad', r, er.first_mismatch(got, emu if cls == 2 else f32(ref)))
    _report('stem %s %s' % (('int', 'onehot', 'rand')[cls], c.name), ratios)


@pytest.mark.parametrize('cls', [0, 1, 2], ids=['int', 'onehot', 'rand'])
@pytest.mark.parametrize('c', er.STEM_CASES, ids=_ids)
def test_stem(abi, c, cls):
    _stem_case(abi, c, cls)


@pytest.mark.parametrize('cls', [0, 1, 2], ids=['int', 'onehot', 'rand'])
def test_stem_2048_block_cap(abi, cls):
    """The one large case: 1 x 1 x 1456 x 1456, k = 1, Cout = 8: 2071 blocks asked, 2048 granted, the last owns no pixel."""
    _stem_case(abi, er.STEM_BIG, cls)


@pytest.mark.parametrize('name', ['k3c32_s2_same', 'k5c40_s2_p1212', 'ow2_s2_same'])
def test_stem_one_nan_reaches_exactly_what_its_taps_reach(abi, name):
    c = STEM[name]
    pt, _, pl, _ = c.pads
    x, w, dy = er.stem_rand_data(c)
    ones_w = np.ones_like(w); ones_x = np.ones_like(x); ones_dy = np.ones_like(dy)
    for site in ((c.N - 1, c.H - 1, c.W - 1, c.Cin - 1), (0, c.H // 2, c.W // 2, 0)):
        ind = np.zeros_like(x); ind[site] = 1
        xn = x.copy(); xn[site] = np.nan
        want = er.stem_fwd_ref(ind, ones_w, c.stride, pt, pl, c.OH, c.OW) > 0
        assert (np.isnan(_stem_fwd(abi, c, xn, w)) == want).all(), 'forward: NaN at x%s' % (site,)
        want = er.stem_wgrad_ref(ind, ones_dy, c.KH, c.KW, c.stride, pt, pl) > 0
        assert (np.isnan(_stem_wgrad(abi, c, xn, dy, runs=1)) == want).all(), 'weight gradient: NaN at x%s' % (site,)
    for site in ((c.N - 1, c.OH - 1, c.OW - 1, c.Cout - 1), (0, c.OH // 2, c.OW // 2, 3)):
        ind = np.zeros_like(dy); ind[site] = 1
        dn = dy.copy(); dn[site] = np.nan
        want = er.stem_wgrad_ref(ones_x, ind, c.KH, c.KW, c.stride, pt, pl) > 0
        assert (np.isnan(_stem_wgrad(abi, c, x, dn, runs=1)) == want).all(), 'weight gradient: NaN at dy%s' % (site,)
        want = er.stem_dgrad_ref(ind, ones_w, c.H, c.W, c.stride, pt, pl) > 0
        assert (np.isnan(_stem_dgrad(abi, c, dn, w)) == want).all(), 'input gradient: NaN at dy%s' % (site,)


# ----------------------------------------------------------------------------- 5. converts and the bf16 add
@pytest.mark.parametrize('c', er.ROWS_CASES, ids=_ids)
def test_converts_and_add(abi, c):
    a, a_bf, b_bf = er.rows_data(c)
    la, lb, lo = c.lds
    src = abi.rows(c.P, c.C, la, False, a)
    dst = abi.rows(c.P, c.C, lo, True)
    abi.call('ssg_convert_f32_to_bf16', src.ptr(), la, c.P, c.C, dst.ptr(), lo)
    got = dst.values((c.P, c.C))
    assert er.same_bits(got, er.convert_ref(a, True)), er.first_mismatch(got, er.convert_ref(a, True))
    assert dst.neighbours_untouched()
    sb = abi.rows(c.P, c.C, lb, True, a_bf)
    df = abi.rows(c.P, c.C, la, False)
    abi.call('ssg_convert_bf16_to_f32', sb.ptr(), lb, c.P, c.C, df.ptr(), la)
    got = df.values((c.P, c.C))
    assert er.same_bits(got, er.convert_ref(a_bf, False)), er.first_mismatch(got, a_bf)
    assert df.neighbours_untouched()
    ar, br = abi.rows(c.P, c.C, la, True, a_bf), abi.rows(c.P, c.C, lb, True, b_bf)
    out = abi.rows(c.P, c.C, lo, True)
    abi.call('ssg_add_bf16', ar.ptr(), la, br.ptr(), lb, c.P, c.C, out.ptr(), lo)
    got = out.values((c.P, c.C))
    assert er.same_bits(got, er.add_ref(a_bf, b_bf)), er.first_mismatch(got, er.add_ref(a_bf, b_bf))
    assert out.neighbours_untouched()
    # finite data only: an element left unwritten keeps its NaN and shows
    fin = f32(np.where(np.isfinite(a), a, 1.5))
    src = abi.rows(c.P, c.C, la, False, fin)
    dst = abi.rows(c.P, c.C, lo, True)
    abi.call('ssg_convert_f32_to_bf16', src.ptr(), la, c.P, c.C, dst.ptr(), lo)
    assert er.same_bits(dst.values((c.P, c.C)), er.bf16_rne(fin))


# ----------------------------------------------------------------------------- 6. assembled: bf16.conv1x1, conv_thin, to_bf16 / to_f32, add
def _bf_nchw(dev, a):
    """[n, h, w, c] values -> the bf16 channels_last tensor [n, c, h, w] the package works on."""
    return torch.from_numpy(f32(a)).to(dev).to(BF).permute(0, 3, 1, 2)


def _nhwc(t):
    return _np(t.permute(0, 2, 3, 1))


def test_conv1x1_autograd(pkg, dev):
    """Integer class through bf16.conv1x1: forward, the transposed pack in backward (input gradient) and the weight gradient, each
    the exact result rounded once; 2 x 9 x 11 pixels, 40 -> 24 channels."""
    n, h, w_, K, N = 2, 9, 11, 40, 24
    rng = np.random.RandomState(11)
    x = f32(rng.randint(0, 16, (n, h, w_, K))); W = f32(rng.randint(-15, 16, (N, K))); dy = f32(rng.randint(-15, 16, (n, h, w_, N)))
    xt = _bf_nchw(dev, x).requires_grad_(True)
    wt = torch.nn.Parameter(torch.from_numpy(W).to(dev).view(N, K, 1, 1))
    y = pkg.bf16.conv1x1(xt, wt)
    assert y.dtype == BF
    assert er.same_bits(_nhwc(y).reshape(-1, N), er.bf16_rne(f32(er.gemm_ref(x.reshape(-1, K), W))))
    y.backward(_bf_nchw(dev, dy))
    assert er.same_bits(_nhwc(xt.grad).reshape(-1, K), er.bf16_rne(f32(er.gemm_ref(dy.reshape(-1, N), W.T))))
    assert wt.grad.dtype == torch.float32 and er.same_bits(_np(wt.grad).reshape(N, K), f32(er.gemm_wgrad_ref(dy.reshape(-1, N), x.reshape(-1, K))))


def test_conv_thin_autograd(pkg, dev):
    c = STEM['k3c32_s2_same']
    pt, _, pl, _ = c.pads
    x, w, dy = er.stem_int_data(c)
    xt = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 3, 1, 2))).to(dev).requires_grad_(True)
    wt = torch.nn.Parameter(torch.from_numpy(w).to(dev))
    y = pkg.bf16.conv_thin(xt, wt, c.stride, c.pads)
    assert y.dtype == BF and tuple(y.shape) == (c.N, c.Cout, c.OH, c.OW)
    assert er.same_bits(_nhwc(y), er.bf16_rne(f32(er.stem_fwd_ref(x, w, c.stride, pt, pl, c.OH, c.OW))))
    y.backward(_bf_nchw(dev, dy))
    assert er.same_bits(_np(wt.grad), f32(er.stem_wgrad_ref(x, dy, c.KH, c.KW, c.stride, pt, pl)))
    assert er.same_bits(_nhwc(xt.grad), f32(er.stem_dgrad_ref(dy, w, c.H, c.W, c.stride, pt, pl)))


def test_convert_round_trip_and_backward(pkg, dev):
    """to_f32(to_bf16(x)) is bf16_rne(x) bit for bit, and so is the gradient that comes back through both converts."""
    rng = np.random.RandomState(12)
    x = f32(np.exp2(rng.uniform(-4, 4, (2, 5, 7, 24))) * rng.choice([-1.0, 1.0], (2, 5, 7, 24)))
    x.reshape(-1)[::9] = f32(1 + 2.0 ** -8)
    x.reshape(-1)[4::9] = f32(1 + 3 * 2.0 ** -8)
    g = f32(x[::-1] * 3)
    xt = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 3, 1, 2))).to(dev).requires_grad_(True)
    y = pkg.bf16.to_f32(pkg.bf16.to_bf16(xt))
    assert y.dtype == torch.float32 and er.same_bits(_nhwc(y), er.bf16_rne(x))
    y.backward(torch.from_numpy(np.ascontiguousarray(g.transpose(0, 3, 1, 2))).to(dev))
    assert er.same_bits(_nhwc(xt.grad), er.bf16_rne(g))
    # each convert's own backward: bf16 -> (to_f32) -> loss gives a bf16 gradient rounded once; fp32 -> (to_bf16) gives fp32 of the bf16 gradient
    b = _bf_nchw(dev, er.bf16_rne(x)).requires_grad_(True)
    pkg.bf16.to_f32(b).backward(torch.from_numpy(np.ascontiguousarray(g.transpose(0, 3, 1, 2))).to(dev))
    assert b.grad.dtype == BF and er.same_bits(_nhwc(b.grad), er.bf16_rne(g))
    xt2 = xt.detach().clone().requires_grad_(True)
    pkg.bf16.to_bf16(xt2).backward(_bf_nchw(dev, er.bf16_rne(g)))
    assert xt2.grad.dtype == torch.float32 and er.same_bits(_nhwc(xt2.grad), er.bf16_rne(g))


def test_add_autograd(pkg, dev):
    c = er.case('rows', 'c40_blocks')
    _, a_bf, b_bf = er.rows_data(c)
    a_bf = np.where(np.isfinite(a_bf), a_bf, 2.0).astype(F32); b_bf = np.where(np.isfinite(b_bf), b_bf, -3.0).astype(F32)
    a = _bf_nchw(dev, a_bf.reshape(1, 7, 43, 40)).requires_grad_(True)
    b = _bf_nchw(dev, b_bf.reshape(1, 7, 43, 40)).requires_grad_(True)
    y = pkg.bf16.add(a, b)
    assert er.same_bits(_nhwc(y).reshape(-1, 40), er.add_ref(a_bf, b_bf))
    g = _bf_nchw(dev, b_bf.reshape(1, 7, 43, 40))
    y.backward(g)
    assert er.same_bits(_nhwc(a.grad).reshape(-1, 40), b_bf) and er.same_bits(_nhwc(b.grad).reshape(-1, 40), b_bf)


def test_pack_cache_follows_the_weight(pkg, dev):
    """conv1x1 reuses one pack object while the weight is unchanged, and repacks after an in-place update (version bump) and after a
    write through .data followed by ops.bump_weight_epoch(); a .data write alone is invisible (the documented reason for the epoch)."""
    n, h, w_, K, N = 1, 4, 5, 16, 8
    rng = np.random.RandomState(13)
    x = f32(rng.randint(0, 16, (n, h, w_, K))); W = f32(rng.randint(-7, 8, (N, K)))
    xt = _bf_nchw(dev, x)
    wt = torch.nn.Parameter(torch.from_numpy(W).to(dev).view(N, K, 1, 1))

    def run():
        return _nhwc(pkg.bf16.conv1x1(xt, wt)).reshape(-1, N), wt._ssg_pack_bf16[1][0]

    def want(Wn):
        return er.bf16_rne(f32(er.gemm_ref(x.reshape(-1, K), Wn)))
    y0, p0 = run()
    y1, p1 = run()
    assert p1 is p0 and er.same_bits(y0, want(W)) and er.same_bits(y1, want(W))
    with torch.no_grad():
        wt.mul_(2)
    y2, p2 = run()
    assert p2 is not p0 and er.same_bits(y2, want(2 * W))
    W3 = f32(W[::-1] + 1)
    wt.data.copy_(torch.from_numpy(np.ascontiguousarray(W3)).view(N, K, 1, 1))
    y3, p3 = run()
    assert p3 is p2 and er.same_bits(y3, want(2 * W))        # the write left no trace on the tensor: the stale pack is reused ...
    pkg.ops.bump_weight_epoch()                              # ... until the epoch moves
    y4, p4 = run()
    assert p4 is not p2 and er.same_bits(y4, want(W3))
