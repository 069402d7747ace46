"""References, emulations, gates and case tables for the bf16 encoder kernels (BASELINE config 4): csrc/gemm_bf16.hip
(ssg_gemm_bf16, ssg_gemm_wgrad_bf16 and its two slab reducers, ssg_pack_weights_bf16), csrc/conv_stem_bf16.hip
(ssg_conv2d_thin_bf16, _wgrad, _dgrad) and ssg_convert_f32_to_bf16 / ssg_convert_bf16_to_f32 / ssg_add_bf16.  numpy only: no
GPU and no op under test.  tests/test_enc_bf16_ref.py rehearses every gate on the CPU (the clean emulation passes, each planted
defect fails), tests/test_enc_bf16_gpu.py holds the kernels to the same gates.

1. references in fp64, written from the contract in include/ssunet_hip.h, not from the kernels
2. bf16_rne: bit-exact round to nearest even with +-Inf, NaN and overflow
3. three data classes: (a) integers whose every partial sum is exact in fp32 in any order, so fp32 outputs equal the reference
   bit for bit and bf16 outputs equal bf16_rne(exact sum); (b) one power-of-two product per output against full 8-bit
   mantissas, bitwise: the addressing; (c) full-mantissa random values under a derived per-element gate and an RMS gate
   against emul()
4. emul(): the kernels' arithmetic in float32 with their partition, and the planted defects as keyword switches
5. the host rules restated (splits, reducer, blocks, pixel lanes, grids, workspaces) with each case's values as literals
6. case tables, facts and check_coverage()

Operands of class (c) lie in [2^-4, 2^4) in magnitude (weights scaled by a power of two): no operand, product or partial sum
comes near an fp32 or bf16 subnormal.  What the matrix unit does with subnormals is not part of the contract.

The image's own pad lanes (channels Cin .. 3 of a 4-float pixel) are ZERO, as the NHWC contract says: the stem kernels
multiply them by zero weights, so a NaN there is outside the contract and no case puts one there.  Pixel strides beyond the
pixel (ldx = 8: lanes 4 .. 7) are never read and hold NaN.
"""
import collections

import numpy as np

from bn_ref import bf16_rne as _rne_finite
from bn_ref import bf16_trunc
from conv_ref import _bf16_bits
from resample_ref import same_bits
from wgrad_ref import RMS_MARGIN, rms

F32, F64 = np.float32, np.float64
U32 = 2.0 ** -24            # unit roundoff of fp32


def bf16_half_ulp(a):
    """Half a unit in the last place of bf16 (8 significant bits) at magnitude a: 2^-9 of the top 2^(e+1) of a's binade [2^e, 2^(e+1)),
    i.e. 2^(e-8).  It lies in (2^-9 |a|, 2^-8 |a|]: the most a correctly rounded store can be off (1 + 2^-8 is a tie and goes to 1:
    2^-8 of the value), so it is the one output rounding of every bf16 gate below.  2^-9 |a| itself is met by no rounding store."""
    _, e = np.frexp(np.abs(np.asarray(a, dtype=F64)))
    return np.where(np.asarray(a, dtype=F64) == 0, 0.0, np.exp2(e.astype(F64) - 9.0))

__all__ = ['RMS_MARGIN', 'rms', 'same_bits', 'bf16_trunc', '_bf16_bits']      # the project's helpers, taken by import and handed on


def f32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=F32))


def cdiv(a, b):
    return -(-a // b)


def round_up(a, b):
    return cdiv(a, b) * b


# ============================================================================ 2. bf16 rounding
def bf16_rne(a):
    """fp32 -> the nearest bf16, ties to even, returned as fp32.  +-Inf stay, a finite value at or above 2^128 - 2^119 (3.4e38)
    becomes Inf, every NaN stays a NaN (returned as the canonical quiet NaN of its sign: NaNs are compared as positions)."""
    a = f32(a)
    out = _rne_finite(a).copy()          # the carry out of the mantissa into the exponent is the overflow to Inf; Inf + 0x7FFF stays Inf
    nan = np.isnan(a)
    if nan.any():
        out[nan] = np.nan
    return out


def is_bf16(a):
    a = f32(a)
    fin = np.isfinite(a)
    return not (a.view(np.uint32)[fin] & np.uint32(0xFFFF)).any()


# ============================================================================ 1. references (fp64)
def pack_ref(w, transpose, rows_pad, Kp):
    """ssg_pack_weights_bf16: w fp32 [O][I] -> bf16 [rows_pad][Kp] (as fp32 values); transpose 0: row o holds w[o][:], transpose 1:
    row i holds w[:][i]; rows and columns beyond the matrix are +0."""
    w = f32(w)
    m = w.T if transpose else w
    out = np.zeros((rows_pad, Kp), dtype=F32)
    out[:m.shape[0], :m.shape[1]] = bf16_rne(m)
    return out


def gemm_ref(x, w, res=None, mag=False):
    """out[p][n] = sum_k x[p][k] w[n][k] (+ res[p][n]) in fp64; x [P][K], w [N][K], res [P][N] hold bf16 values.  With mag: also
    sum_k |x w| (+ |res|)."""
    x = np.asarray(x, dtype=F64); w = np.asarray(w, dtype=F64)
    out = x @ w.T
    if res is not None:
        out = out + np.asarray(res, dtype=F64)
    if not mag:
        return out
    m = np.abs(x) @ np.abs(w).T
    if res is not None:
        m = m + np.abs(np.asarray(res, dtype=F64))
    return out, m


def gemm_wgrad_ref(dy, x, mag=False):
    """dw[m][n] = sum_p dy[p][m] x[p][n] in fp64."""
    dy = np.asarray(dy, dtype=F64); x = np.asarray(x, dtype=F64)
    out = dy.T @ x
    return (out, np.abs(dy).T @ np.abs(x)) if mag else out


def _canvas(x, KH, KW, stride, pad_t, pad_l, OH, OW):
    """x [N, H, W, C] fp64 on a zero canvas such that output (oy, ox) tap (ky, kx) is canvas[oy * stride + ky, ox * stride + kx]:
    the image sits at (pad_t, pad_l), the canvas covers the image and every window."""
    N, H, W, C = x.shape
    CH = max((OH - 1) * stride + KH, pad_t + H)
    CW = max((OW - 1) * stride + KW, pad_l + W)
    cv = np.zeros((N, CH, CW, C), dtype=F64)
    cv[:, pad_t:pad_t + H, pad_l:pad_l + W] = x
    return cv


def _tap(cv, ky, kx, stride, OH, OW):
    return cv[:, ky:ky + (OH - 1) * stride + 1:stride, kx:kx + (OW - 1) * stride + 1:stride]


def stem_fwd_ref(x, w, stride, pad_t, pad_l, OH, OW, mag=False, round_x=True):
    """y[n][oy][ox][co] = sum_{c, ky, kx} bf16(x[n][oy s - pad_t + ky][ox s - pad_l + kx][c]) bf16(w[co][c][ky][kx]) in fp64, taps
    outside the image contribute nothing.  x [N, H, W, Cin] fp32 values, w [Cout, Cin, KH, KW]."""
    xr = (bf16_rne(x) if round_x else f32(x)).astype(F64); wr = bf16_rne(w).astype(F64)
    Cout, Cin, KH, KW = wr.shape
    y = np.zeros((x.shape[0], OH, OW, Cout), dtype=F64)
    m = np.zeros_like(y)
    cv = _canvas(xr, KH, KW, stride, pad_t, pad_l, OH, OW)
    for ky in range(KH):
        for kx in range(KW):
            t = _tap(cv, ky, kx, stride, OH, OW)
            y += t @ wr[:, :, ky, kx].T
            if mag:
                m += np.abs(t) @ np.abs(wr[:, :, ky, kx]).T
    return (y, m) if mag else y


def stem_wgrad_ref(x, dy, KH, KW, stride, pad_t, pad_l, mag=False, round_x=True):
    """dw[co][c][ky][kx] = sum over output pixels of dy[n][oy][ox][co] bf16(x[n][oy s - pad_t + ky][ox s - pad_l + kx][c])."""
    xr = (bf16_rne(x) if round_x else f32(x)).astype(F64); d = np.asarray(dy, dtype=F64)
    N, OH, OW, Cout = d.shape
    Cin = x.shape[3]
    dw = np.zeros((Cout, Cin, KH, KW), dtype=F64)
    m = np.zeros_like(dw)
    cv = _canvas(xr, KH, KW, stride, pad_t, pad_l, OH, OW)
    d2 = d.reshape(-1, Cout)
    for ky in range(KH):
        for kx in range(KW):
            t = np.ascontiguousarray(_tap(cv, ky, kx, stride, OH, OW)).reshape(-1, Cin)
            dw[:, :, ky, kx] = d2.T @ t
            if mag:
                m[:, :, ky, kx] = np.abs(d2).T @ np.abs(t)
    return (dw, m) if mag else dw


def stem_dgrad_ref(dy, w, H, W, stride, pad_t, pad_l, mag=False):
    """dx[n][iy][ix][c] = sum over (ky, kx, co) with iy = oy s - pad_t + ky, ix = ox s - pad_l + kx of dy[n][oy][ox][co] bf16(w[co][c][ky][kx])."""
    d = np.asarray(dy, dtype=F64); wr = bf16_rne(w).astype(F64)
    N, OH, OW, Cout = d.shape
    _, Cin, KH, KW = wr.shape
    cv = _canvas(np.zeros((N, H, W, Cin), dtype=F64), KH, KW, stride, pad_t, pad_l, OH, OW)
    cm = np.zeros_like(cv)
    for ky in range(KH):
        for kx in range(KW):
            _tap(cv, ky, kx, stride, OH, OW)[...] += d @ wr[:, :, ky, kx]
            if mag:
                _tap(cm, ky, kx, stride, OH, OW)[...] += np.abs(d) @ np.abs(wr[:, :, ky, kx])
    dx = np.ascontiguousarray(cv[:, pad_t:pad_t + H, pad_l:pad_l + W])
    return (dx, np.ascontiguousarray(cm[:, pad_t:pad_t + H, pad_l:pad_l + W])) if mag else dx


def convert_ref(a, to_bf16):
    """fp32 -> bf16 is one rounding to nearest even; bf16 -> fp32 is exact."""
    return bf16_rne(a) if to_bf16 else f32(a)


def add_ref(a, b):
    """out = bf16(fp32(a + b)) on bf16 values: the sum is formed in fp32 (exact whenever the exponents lie within 16 of each
    other, as in every case here) and rounded once to bf16."""
    with np.errstate(invalid='ignore', over='ignore'):
        return bf16_rne((np.asarray(a, dtype=F64) + np.asarray(b, dtype=F64)).astype(F32))


# ============================================================================ 5. host rules restated
GB_M = GB_N = 128
FWD_ITEMS = 16
STEM_MAX_BLOCKS = 2048
REDUCE_SERIAL, REDUCE_32 = 'serial', 'reduce32'


def gemm_plan(P, K, N):
    """(tiles, nsteps, column tiles) of ssg_gemm_bf16."""
    return cdiv(N, GB_N) * cdiv(P, GB_M), cdiv(K, 32), cdiv(N, GB_N)


def wg_splits(P, M, N):
    tiles = cdiv(M, 128) * cdiv(N, 128)
    nk = cdiv(P, 32)
    slab = M * N * 4
    target = 2048 if slab <= (64 << 10) else (1024 if slab <= (512 << 10) else 512)
    s = min(target // tiles, nk // 8)
    return max(1, min(s, 2048))


def wg_plan(P, M, N):
    """(splits, steps per split, splits that own no step, reducer, workspace bytes) of ssg_gemm_wgrad_bf16."""
    s = wg_splits(P, M, N)
    nk = cdiv(P, 32)
    sps = cdiv(nk, s)
    empty = s - cdiv(nk, sps)
    red = REDUCE_32 if (s >= 64 and M * N <= (1 << 18)) else REDUCE_SERIAL
    return s, sps, empty, red, s * M * N * 4


def stem_blocks(P):
    return max(1, min(cdiv(P, 1024), STEM_MAX_BLOCKS))


def stem_plan(N, OH, OW, Cout, KH, KW):
    """(blocks, per_block, WG_PL, forward items, forward grid, weight-gradient workspace bytes)."""
    P = N * OH * OW
    b = stem_blocks(P)
    groups = KH * KW * (Cout // 8)
    items = P * (Cout // 8)
    return b, cdiv(P, b), min(4, 256 // groups), items, cdiv(items, 256 * FWD_ITEMS), b * KH * KW * Cout * 16


# ============================================================================ 6. case tables
GemmCase = collections.namedtuple('GemmCase', 'name P K N transpose Kp nan_rows tiles nsteps facts')
WgCase = collections.namedtuple('WgCase', 'name P M N splits sps empty reducer ws_bytes facts')
StemCase = collections.namedtuple('StemCase', 'name N Cin H W Cout KH KW stride pads OH OW ldx ldy blocks per_block wg_pl items grid ws_bytes facts')
RowsCase = collections.namedtuple('RowsCase', 'name P C lds facts')


def _g(name, P, K, N, tiles, nsteps, facts, transpose=0, Kp=None, nan_rows=False):
    facts = set(facts) | {'ld_gaps', 'res_on_off'}
    return GemmCase(name, P, K, N, transpose, Kp or round_up(K, 32), nan_rows, tiles, nsteps, frozenset(facts))


# strides of every GEMM case: ldx = K + 8, ldo = N + 8, ldr = N + 16 (gaps NaN); weight gradient: ldd = M + 8, ldx = N + 16
GEMM_CASES = [
    _g('p1_k8_n8', 1, 8, 8, 1, 1, {'P=1', 'tail8', 'tiles<8', 'nsteps1'}),
    _g('p127_k24_n120', 127, 24, 120, 1, 1, {'tail24', 'nan_pack_rows', 'nsteps1'}, nan_rows=True),
    _g('p128_k32_n128', 128, 32, 128, 1, 1, {'full_tile', 'nsteps1'}),
    _g('p129_k40_n136', 129, 40, 136, 4, 2, {'tail8', 'nsteps2', 'col_tiles2', 'Kp+32'}, Kp=96),
    _g('p127_k48_n8_t', 127, 48, 8, 1, 2, {'tail16', 'transpose', 'nsteps2'}, transpose=1),
    _g('t7_k64_n8', 895, 64, 8, 7, 2, {'tiles7', 'tiles<8', 'nsteps2'}),
    _g('t8_k72_n120', 1024, 72, 120, 8, 3, {'tiles8', 'remap_full', 'nsteps3', 'ring_wrap', 'tail8'}),
    _g('t9_k96_n128', 1025, 96, 128, 9, 3, {'tiles9', 'remap_tail', 'nsteps3', 'ring_wrap'}),
    _g('t19_k104_n8', 2400, 104, 8, 19, 4, {'tiles19', 'remap_tail', 'nsteps4', 'ring_wrap', 'tail8'}),
    _g('t12_k136_n136_t', 700, 136, 136, 12, 5, {'tiles12', 'col_tiles2', 'remap_tail', 'nsteps5', 'tail8', 'transpose'}, transpose=1),
    _g('p129_k672_n264_t', 129, 672, 264, 6, 21, {'col_tiles3', 'nsteps21', 'transpose', 'K=672'}, transpose=1),
]


def _w(name, P, M, N, splits, sps, empty, reducer, facts):
    return WgCase(name, P, M, N, splits, sps, empty, reducer, splits * M * N * 4, frozenset(set(facts) | {'ld_gaps'}))


WG_CASES = [
    _w('p1_8x8', 1, 8, 8, 1, 1, 0, REDUCE_SERIAL, {'P=1', 'one_split'}),
    _w('p31_24x8', 31, 24, 8, 1, 1, 0, REDUCE_SERIAL, {'P<32'}),
    _w('p32_8x24', 32, 8, 24, 1, 1, 0, REDUCE_SERIAL, {'P=32'}),
    _w('p33_24x24', 33, 24, 24, 1, 2, 0, REDUCE_SERIAL, {'P=33'}),
    _w('p255_128x136', 255, 128, 136, 1, 8, 0, REDUCE_SERIAL, {'tiles2', 'ring_wrap'}),
    _w('p256_136x128', 256, 136, 128, 1, 8, 0, REDUCE_SERIAL, {'tiles2', 'ring_wrap'}),
    _w('p512_264x8', 512, 264, 8, 2, 8, 0, REDUCE_SERIAL, {'tiles3', 'splits2'}),
    _w('p4133_24x264', 4133, 24, 264, 16, 9, 1, REDUCE_SERIAL, {'empty_split', 'tiles3', 'ragged_P'}),
    _w('p4133_8x8', 4133, 8, 8, 16, 9, 1, REDUCE_SERIAL, {'empty_split', 'ragged_P'}),
    _w('p16352_8x24', 16352, 8, 24, 63, 9, 6, REDUCE_SERIAL, {'splits63', 'empty_split'}),
    _w('p16400_24x8', 16400, 24, 8, 64, 9, 7, REDUCE_32, {'splits64', 'reduce32', 'empty_split'}),
    _w('p20000_112x672', 20000, 112, 672, 78, 9, 8, REDUCE_32, {'reduce32', 'empty_split', 'tiles6', 'splits78'}),
    _w('p524320_8x8', 524320, 8, 8, 2048, 9, 227, REDUCE_32, {'split_cap', 'reduce32', 'empty_split'}),
]


def _s(name, N, Cin, H, W, Cout, KH, KW, stride, pads, OH, OW, blocks, per_block, wg_pl, items, grid, facts, ldx=8, ld_gap=8):
    return StemCase(name, N, Cin, H, W, Cout, KH, KW, stride, pads, OH, OW, ldx, Cout + ld_gap, blocks, per_block, wg_pl, items, grid,
                    blocks * KH * KW * Cout * 16, frozenset(facts))


# pads = (top, bottom, left, right); ldx = 8 (lanes 4 .. 7 NaN, never read), ldy = lddy = Cout + 8, lddx = 8
STEM_CASES = [
    _s('k3c8_s1', 1, 3, 5, 7, 8, 3, 3, 1, (1, 1, 1, 1), 5, 7, 1, 35, 4, 35, 1, {'pl4', 'one_block', 'items<256', 'sym_pad', 'odd_hw', 'stride1'}),
    _s('k3c32_s2_same', 2, 3, 37, 51, 32, 3, 3, 2, (0, 1, 0, 1), 18, 25, 1, 900, 4, 3600, 1, {'pl4', 'same_pad', 'stride2', 'odd_hw', 'one_block'}),
    _s('k3c48_s2_sym', 3, 3, 31, 29, 48, 3, 3, 2, (1, 1, 1, 1), 16, 15, 1, 720, 4, 4320, 2, {'pl4', 'sym_pad', 'stride2', 'odd_hw', 'ragged_items'}),
    _s('k3c64_s1', 1, 4, 9, 11, 64, 3, 3, 1, (1, 1, 1, 1), 9, 11, 1, 99, 3, 792, 1, {'pl3', 'cin4', 'stride1', 'odd_hw'}),
    _s('k5c40_s2_p1212', 1, 4, 21, 25, 40, 5, 5, 2, (1, 2, 1, 2), 10, 12, 1, 120, 2, 600, 1, {'pl2', 'k5', 'pad1212', 'cin4', 'stride2', 'odd_hw'}),
    _s('k5c56_s1', 1, 3, 7, 9, 56, 5, 5, 1, (2, 2, 2, 2), 7, 9, 1, 63, 1, 441, 1, {'pl1', 'k5', 'stride1', 'odd_hw'}),
    _s('k1c8_cin1', 2, 1, 5, 3, 8, 1, 1, 1, (0, 0, 0, 0), 5, 3, 1, 30, 4, 30, 1, {'k1', 'cin1', 'ow3', 'wrap_loop', 'items<256'}),
    _s('k1x3c8', 1, 3, 6, 9, 8, 1, 3, 1, (0, 0, 1, 1), 6, 9, 1, 54, 4, 54, 1, {'k1x3', 'stride1'}),
    _s('ow1_s2', 2, 3, 9, 2, 8, 3, 3, 2, (1, 1, 1, 1), 5, 1, 1, 10, 4, 10, 1, {'ow1', 'wrap_loop', 'stride2'}),
    _s('ow2_s2_same', 1, 3, 11, 4, 16, 3, 3, 2, (0, 1, 0, 1), 5, 2, 1, 10, 4, 20, 1, {'ow2', 'wrap_loop', 'same_pad', 'stride2'}),
    _s('ow3_s1_c64', 2, 3, 7, 3, 64, 3, 3, 1, (1, 1, 1, 1), 7, 3, 1, 42, 3, 336, 1, {'ow3', 'pl3'}),
    _s('items4096', 1, 3, 32, 32, 32, 3, 3, 1, (1, 1, 1, 1), 32, 32, 1, 1024, 4, 4096, 1, {'items4096', 'per_block1024'}),
    _s('b5_c48', 2, 3, 48, 48, 48, 3, 3, 1, (1, 1, 1, 1), 48, 48, 5, 922, 4, 27648, 7, {'blocks2-64', 'ragged_items', 'ragged_blocks'}),
    _s('b72_s2_same', 2, 3, 384, 384, 32, 3, 3, 2, (0, 1, 0, 1), 192, 192, 72, 1024, 4, 294912, 72, {'blocks72', 'second_lap', 'same_pad', 'stride2'}),
]
# the one large case (x 34 MB, dy 34 MB): 2071 blocks asked, 2048 granted, the last one owns no pixel
STEM_BIG = _s('b2048_k1', 1, 1, 1456, 1456, 8, 1, 1, 1, (0, 0, 0, 0), 1456, 1456, 2048, 1036, 4, 2119936, 518, {'block_cap', 'empty_block', 'second_lap', 'k1', 'cin1'},
              ldx=4, ld_gap=0)


def _r(name, P, C, lds, facts):
    return RowsCase(name, P, C, lds, frozenset(facts))


# lds = (a / source stride, b stride, destination stride), all distinct; work items = P C / 4
ROWS_CASES = [
    _r('c4_odd', 5, 4, (8, 12, 16), {'C=4', 'odd_items', 'items<512'}),
    _r('c8_odd_pairs', 63, 8, (16, 24, 12), {'C=8', 'items<512'}),
    _r('c12_odd', 37, 12, (16, 20, 24), {'C=12', 'odd_items', 'items<512'}),
    _r('c40_blocks', 301, 40, (48, 44, 56), {'C=40', 'several_blocks'}),
]

ALL_TABLES = dict(gemm=GEMM_CASES, wgrad=WG_CASES, stem=STEM_CASES + [STEM_BIG], rows=ROWS_CASES)


def case(table, name):
    (c,) = [c for c in ALL_TABLES[table] if c.name == name]
    return c


def _seed(name, cls):
    return (sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) * 7 + cls * 1009) % (2 ** 31)


# ---------------------------------------------------------------------------- data: GEMM forward / input gradient
# A GEMM data set is (x [P][K], W fp32 module weight ([N][K], or [K][N] where the case packs with transpose 1), res [P][N]).
def w_eff(c, W):
    """The [N][K] matrix the GEMM multiplies by, from the module weight as the case lays it out."""
    return np.ascontiguousarray(f32(W).T) if c.transpose else f32(W)


def _lay(c, weff):
    return np.ascontiguousarray(weff.T) if c.transpose else weff


def full_mantissa(idx):
    """Distinct bf16 values with full 8-bit mantissas: (128 + idx mod 128) 2^(e - 7), e cycling through -4 .. 3, sign alternating
    every 1024: any 2048 consecutive sites hold different values, and none is near a subnormal."""
    idx = np.asarray(idx, dtype=np.int64)
    m = 128 + idx % 128
    e = (idx // 128) % 8 - 4
    s = 1 - 2 * ((idx // 1024) % 2)
    return f32(s * m * np.exp2(e - 7.0))


def gemm_int_data(c):
    rng = np.random.RandomState(_seed(c.name, 0))
    x = f32(rng.randint(0, 16, (c.P, c.K)))                  # 0 .. 15, w -15 .. 15, res -64 .. 64: sum |terms| <= 225 K + 64
    w = f32(rng.randint(-15, 16, (c.N, c.K)))
    res = f32(rng.randint(-64, 65, (c.P, c.N)))
    return x, _lay(c, w), res


def gemm_onehot_data(c, variant):
    """w[n][sigma(n)] = +-2^e, everything else zero; x full mantissas distinct per (pixel, channel): out[p][n] = x[p][sigma(n)] 2^e."""
    w = np.zeros((c.N, c.K), dtype=F32)
    n = np.arange(c.N)
    sig = (n * (5 + 2 * variant) + 3 + variant) % c.K
    w[n, sig] = f32((1 - 2 * (n % 2)) * np.exp2((n + variant) % 5 - 2.0))
    x = full_mantissa(np.arange(c.P * c.K)).reshape(c.P, c.K)
    return x, _lay(c, w), None


def _rand_bf16(rng, shape, scale=1.0):
    """Full-mantissa values of magnitude [2^-4, 2^4) times `scale` (a power of two), random sign, rounded to bf16."""
    v = np.exp2(rng.uniform(-4, 4, shape)) * rng.choice([-1.0, 1.0], shape)
    return f32(bf16_rne(f32(v)) * scale)


def gemm_rand_data(c):
    rng = np.random.RandomState(_seed(c.name, 2))
    x = _rand_bf16(rng, (c.P, c.K))
    w = _rand_bf16(rng, (c.N, c.K), 2.0 ** -3)
    res = _rand_bf16(rng, (c.P, c.N))
    return x, _lay(c, w), res


# ---------------------------------------------------------------------------- data: GEMM weight gradient (dy [P][M], x [P][N])
def wg_int_range(c):
    return int(min(15, np.floor(np.sqrt((2 ** 24 - 1) / c.P))))


def wg_int_data(c):
    rng = np.random.RandomState(_seed(c.name, 0))
    a = wg_int_range(c)
    return f32(rng.randint(-a, a + 1, (c.P, c.M))), f32(rng.randint(-a, a + 1, (c.P, c.N)))


def wg_onehot_data(c, variant):
    """dy[pi(m)][m] = +-2^e at one pixel per row m of dw; x full mantissas: dw[m][n] = 2^e x[pi(m)][n]."""
    dy = np.zeros((c.P, c.M), dtype=F32)
    m = np.arange(c.M)
    pi = (m * (7919 + 2 * variant) + 13 + variant * (c.P // 2)) % c.P
    if variant == 1:
        pi[-1] = c.P - 1                                    # the last pixel: the ragged K-step, the last non-empty split
    dy[pi, m] = f32((1 - 2 * (m % 2)) * np.exp2(m % 5 - 2.0))
    return dy, full_mantissa(np.arange(c.P * c.N)).reshape(c.P, c.N)


def wg_rand_data(c):
    rng = np.random.RandomState(_seed(c.name, 2))
    return _rand_bf16(rng, (c.P, c.M)), _rand_bf16(rng, (c.P, c.N))


# ---------------------------------------------------------------------------- data: stem (x [N,H,W,Cin] fp32, w OIHW fp32, dy [N,OH,OW,Cout] bf16)
def stem_int_range(c):
    return int(min(15, np.floor(np.sqrt((2 ** 24 - 1) / (c.N * c.OH * c.OW)))))


def stem_int_data(c):
    rng = np.random.RandomState(_seed(c.name, 0))
    a = stem_int_range(c)
    x = f32(rng.randint(-a, a + 1, (c.N, c.H, c.W, c.Cin)))
    w = f32(rng.randint(-a, a + 1, (c.Cout, c.Cin, c.KH, c.KW)))
    dy = f32(rng.randint(-a, a + 1, (c.N, c.OH, c.OW, c.Cout)))
    return x, w, dy


def stem_rand_data(c):
    """x and w carry full fp32 mantissas (the kernels round them to bf16 themselves); dy is a bf16 tensor."""
    rng = np.random.RandomState(_seed(c.name, 2))
    x = f32(np.exp2(rng.uniform(-4, 4, (c.N, c.H, c.W, c.Cin))) * rng.choice([-1.0, 1.0], (c.N, c.H, c.W, c.Cin)))
    w = f32(np.exp2(rng.uniform(-4, 4, (c.Cout, c.Cin, c.KH, c.KW))) * rng.choice([-1.0, 1.0], (c.Cout, c.Cin, c.KH, c.KW)) * 2.0 ** -3)
    dy = _rand_bf16(rng, (c.N, c.OH, c.OW, c.Cout))
    return x, w, dy


def stem_onehot_data(c, op, variant):
    """op 'fwd': one weight +-2^e per output channel at (c, ky, kx)(co), x full mantissas per (pixel, channel).
    op 'wgrad': dy one +-2^e per output channel at pixel pi(co), x full mantissas.
    op 'dgrad': one weight per INPUT channel at (co, ky, kx)(c), dy full mantissas.  Every output is one exact product."""
    nt = c.KH * c.KW
    x = full_mantissa(np.arange(c.N * c.H * c.W * c.Cin)).reshape(c.N, c.H, c.W, c.Cin)
    dy = full_mantissa(np.arange(c.N * c.OH * c.OW * c.Cout)).reshape(c.N, c.OH, c.OW, c.Cout)
    w = np.zeros((c.Cout, c.Cin, nt), dtype=F32)
    co = np.arange(c.Cout)
    if op == 'fwd':
        w[co, (co + variant) % c.Cin, (co * 2 + variant) % nt] = f32((1 - 2 * (co % 2)) * np.exp2(co % 5 - 2.0))
    elif op == 'dgrad':
        ci = np.arange(c.Cin)
        w[(ci * 3 + variant) % c.Cout, ci, (ci * 2 + variant * 4) % nt] = f32((1 - 2 * (ci % 2)) * np.exp2(ci - 1.0))
    else:
        P = c.N * c.OH * c.OW
        d = np.zeros((P, c.Cout), dtype=F32)
        pi = (co * (7919 + 2 * variant) + 13 + variant * (P // 2)) % P
        if variant == 1:
            pi[-1] = P - 1
        d[pi, co] = f32((1 - 2 * (co % 2)) * np.exp2(co % 5 - 2.0))
        dy = d.reshape(c.N, c.OH, c.OW, c.Cout)
    return x, w.reshape(c.Cout, c.Cin, c.KH, c.KW), dy


# ---------------------------------------------------------------------------- data: converts / add
SPECIALS_F32 = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 3.4e38, -3.4e38, 3.39e38, 257.0, 259.0, -257.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8,
                         1.0 + 2.0 ** -8 + 2.0 ** -23, 1.0 + 2.0 ** -8 - 2.0 ** -24, 1.00390625, 65280.0 + 128.0], dtype=F32)


def rows_data(c, integer=False):
    """(a fp32 [P][C] with the special values spread through it, a_bf, b_bf): a holds full fp32 mantissas; ties (257, 259,
    1 + 2^-8 ...), +-Inf, NaN, +-0 and 3.4e38 (bf16 Inf) sit at fixed places; a_bf + b_bf covers Inf - Inf and ties 256 + 1."""
    rng = np.random.RandomState(_seed(c.name, 3))
    n = c.P * c.C
    a = f32(np.exp2(rng.uniform(-4, 4, n)) * rng.choice([-1.0, 1.0], n))
    pos = (np.arange(len(SPECIALS_F32)) * 7 + 3) % n
    if n > len(SPECIALS_F32) * 7:
        a[pos] = SPECIALS_F32
    else:
        a[:min(n, len(SPECIALS_F32))] = SPECIALS_F32[:n]
    a_bf = bf16_rne(a)
    b_bf = f32(rng.randint(-3, 4, n) * 2 + 1)              # odd integers: against 256 / 258 ... they make ties
    ties = (np.arange(n) % 5 == 0) & np.isfinite(a_bf)
    a_bf = a_bf.copy(); a_bf[ties] = f32(256 + 2 * (np.arange(n)[ties] % 64))
    b_bf[(np.arange(n) % 11 == 1)] = np.inf
    b_bf[(np.arange(n) % 13 == 2)] = -np.inf
    return a.reshape(c.P, c.C), a_bf.reshape(c.P, c.C), b_bf.reshape(c.P, c.C)


# ============================================================================ 3. exactness of the integer class
def int_class_is_exact(c, data=None):
    """The integer data of case c has sum |terms| < 2^24 at every output of every operation it feeds, so every product and every
    partial sum in any order is an integer below 2^24: exact in fp32.  Computed from the data themselves, per case."""
    lim = 2.0 ** 24
    if isinstance(c, GemmCase):
        x, W, res = data or gemm_int_data(c)
        _, m = gemm_ref(x, w_eff(c, W), res, mag=True)
        return is_bf16(x) and is_bf16(W) and is_bf16(res) and float(m.max()) < lim
    if isinstance(c, WgCase):
        dy, x = data or wg_int_data(c)
        _, m = gemm_wgrad_ref(dy, x, mag=True)
        return is_bf16(dy) and is_bf16(x) and float(m.max()) < lim
    if isinstance(c, StemCase):
        x, w, dy = data or stem_int_data(c)
        pt, _, pl, _ = c.pads
        m1 = stem_fwd_ref(x, w, c.stride, pt, pl, c.OH, c.OW, mag=True)[1]
        m2 = stem_wgrad_ref(x, dy, c.KH, c.KW, c.stride, pt, pl, mag=True)[1]
        m3 = stem_dgrad_ref(dy, w, c.H, c.W, c.stride, pt, pl, mag=True)[1]
        return is_bf16(x) and is_bf16(w) and is_bf16(dy) and max(float(m1.max()), float(m2.max()), float(m3.max())) < lim
    raise TypeError(c)


def has_ties(ref):
    """Does the exact fp64 result hold a value a truncating (or half-away) bf16 store would round differently?"""
    r = f32(ref)
    return bool((bf16_rne(r) != bf16_trunc(r)).any()), bool(((np.abs(r) >= 256) & (np.abs(r) < 512) & (np.abs(r) % 2 == 1)).any())


# ============================================================================ gates of class (c)
# Every gate: (number of fp32 roundings on the path to one output) x u32 x (magnitude sum of the fp64 reference), plus the store.
#
# GEMM forward: the 32 products of a K-step enter two 16-deep MFMAs; a matrix unit sums its 16 exact products (bf16 x bf16 has 16
# significant bits) and the fp32 accumulator and rounds once: 2 nsteps roundings of a partial sum bounded by mag.  One more u32 mag
# covers an MFMA that rounds its internal sum to within an ulp instead of half, one more the fp32 `+ res` and the second order.
# The bf16 store rounds the computed fp32 value: half a bf16 ulp at |ref| + fp32 error.
def gemm_gate(c, ref, mag):
    e32 = (2 * c.nsteps + 2) * U32 * np.asarray(mag, dtype=F64)
    return e32 + bf16_half_ulp(np.abs(ref) + e32)


# GEMM weight gradient: a split's accumulator takes 2 sps MFMAs; the serial reducer adds `splits` slabs, reduce32 ceil(splits / 32)
# + 5: both at most `splits`.  (2 sps + splits) roundings of partial sums bounded by mag, + 2 u32 mag as above; the result is stored
# as fp32, the last addition's rounding is already counted.
def wg_gate(c, ref, mag):
    return (2 * c.sps + c.splits + 2) * U32 * np.asarray(mag, dtype=F64)


# Stem forward: one fma per (tap, input channel) into an fp32 accumulator: KH KW Cin roundings (pad lanes add an exact zero); then the
# bf16 store.  Input gradient: one fma per (tap, output channel) that reaches the pixel: at most KH KW Cout.  Weight gradient: a
# thread multiplies (one rounding unless contracted) and adds (one rounding) for each of its ceil(per_block / WG_PL) pixels, lane 0
# adds WG_PL - 1 lane sums; the blocks are summed in fp64 (2^-53: nothing) and stored as fp32: u32 |ref|.
def stem_fwd_gate(c, ref, mag):
    e32 = (c.KH * c.KW * c.Cin + 1) * U32 * np.asarray(mag, dtype=F64)
    return e32 + bf16_half_ulp(np.abs(ref) + e32)


def stem_dgrad_gate(c, ref, mag):
    return (c.KH * c.KW * c.Cout + 1) * U32 * np.asarray(mag, dtype=F64)


def stem_wgrad_gate(c, ref, mag):
    return (2 * cdiv(c.per_block, c.wg_pl) + c.wg_pl + 1) * U32 * np.asarray(mag, dtype=F64) + U32 * np.abs(ref)


def worst(got, ref, gate):
    """max |got - ref| / gate over the tensor; a NaN or Inf in `got` where the reference is finite is infinitely wrong."""
    got = np.asarray(got, dtype=F64); ref = np.asarray(ref, dtype=F64)
    if got.shape != ref.shape or not np.isfinite(got).all():
        return float('inf')
    err = np.abs(got - ref)
    gate = np.asarray(gate, dtype=F64)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(err == 0, 0.0, err / gate)
    return float(r.max()) if r.size else 0.0


def rms_ratio(got, emu, ref):
    """RMS error of the kernel over RMS_MARGIN x the emulation's: pass <= 1.  An emulation that is exact where the kernel is not
    gives inf; both exact gives 0."""
    ref = np.asarray(ref, dtype=F64)
    if not np.isfinite(np.asarray(got, dtype=F64)).all():
        return float('inf')
    a = rms(np.asarray(got, dtype=F64) - ref); b = rms(np.asarray(emu, dtype=F64) - ref)
    if a == 0:
        return 0.0
    return float('inf') if b == 0 else a / (RMS_MARGIN * b)


def first_mismatch(got, ref):
    got = f32(got); ref = f32(ref)
    if got.shape != ref.shape:
        return 'shape %s against %s' % (got.shape, ref.shape)
    na, nb = np.isnan(got), np.isnan(ref)
    bad = np.argwhere((na != nb) | (~na & ~nb & (got.view(np.int32) != ref.view(np.int32))))
    if not len(bad):
        return None
    i = tuple(int(v) for v in bad[0])
    return '%d of %d elements differ, first at %s: got %r, reference %r' % (len(bad), got.size, i, got[i], ref[i])


# ============================================================================ 4. emulations (float32, the kernels' partition)
def _acc(acc, part):
    """fp32 accumulator + an exactly known addend, rounded once (the fp64 sum of an fp32 value and a short exact sum of 16-bit
    products is exact at these magnitudes, so this is the single rounding the hardware makes)."""
    return (acc.astype(F64) + part).astype(F32)


def pack_emul(W, transpose, rows_pad, Kp, wrong_transpose=False):
    """pack_ref's result by the kernel's flat index walk.  Defect: the transposed pack read as w[r O + k] instead of w[k I + r]."""
    W = f32(W)
    O, I = W.shape
    rows, cols = (I, O) if transpose else (O, I)
    out = np.zeros((rows_pad, Kp), dtype=F32)
    if transpose and wrong_transpose:
        out[:rows, :cols] = bf16_rne(W.reshape(-1)[:rows * cols].reshape(rows, cols))
    elif transpose:
        out[:rows, :cols] = bf16_rne(W.T)
    else:
        out[:rows, :cols] = bf16_rne(W)
    return out


def gemm_emul(c, x, wp, resbuf=None, ldo=None, truncate=False, drop_last_step=False, tail_chunk_zero=False, swizzle_off=False,
              res_stride_ldo=False, drop_pixel_tail=False, half_away=False):
    """ssg_gemm_bf16 in float32: K-steps of 32 as two 16-deep MFMAs (16 exact products + the fp32 accumulator, one rounding), the
    fp32 `+ res`, the bf16 store.  x [P][K]; wp the pack [rows_pad][Kp] (rows >= N are not read: the kernel takes the zero page
    there); resbuf the residual's whole buffer [P][ldr] with the values in its first N lanes, or None.  Returns [P][N] as fp32.
    Defects: truncating or half-away store; last K-step dropped; the last 8-channel chunk of a K % 32 tail read as zero; the chunk
    swizzle off by one row group (rows with (p >> 2) & 1 take chunk q ^ 1 of each step); res read at stride ldo; pixel row P - 1
    never stored (it keeps the caller's NaN)."""
    P, K, N = c.P, c.K, c.N
    ns = c.nsteps - (1 if drop_last_step else 0)
    xk = np.zeros((P, c.nsteps * 32), dtype=F64); xk[:, :K] = x
    if tail_chunk_zero and K % 32:
        xk[:, K - 8:K] = 0
    if swizzle_off:
        v = xk.reshape(P, c.nsteps, 4, 8).copy()
        odd = ((np.arange(P) >> 2) & 1) == 1
        v[odd] = v[odd][:, :, [1, 0, 3, 2]]
        xk = v.reshape(P, -1)
    wk = np.zeros((N, c.nsteps * 32), dtype=F64); wk[:, :min(c.Kp, c.nsteps * 32)] = np.asarray(wp, dtype=F64)[:N, :c.nsteps * 32]
    acc = np.zeros((P, N), dtype=F32)
    for h in range(2 * ns):
        acc = _acc(acc, xk[:, 16 * h:16 * h + 16] @ wk[:, 16 * h:16 * h + 16].T)
    if resbuf is not None:
        rb = f32(resbuf)
        if res_stride_ldo:
            r = rb.reshape(-1)[(np.arange(P)[:, None] * ldo + np.arange(N)[None, :])]
        else:
            r = rb[:, :N]
        with np.errstate(invalid='ignore'):
            acc = (acc.astype(F64) + r.astype(F64)).astype(F32)
    if truncate:
        out = bf16_trunc(acc)
    elif half_away:
        out = bf16_trunc((acc.view(np.uint32) + np.uint32(0x8000)).view(F32))
    else:
        out = bf16_rne(acc)
    if drop_pixel_tail:
        out = out.copy(); out[P - 1] = np.nan
    return out


def wg_reduce_emul(slabs, reducer, stop_after=None):
    """The ordered slab sum: serial (one thread adds slab 0, 1, ...) or reduce32 (lane k adds slabs k, k + 32, ... in order, then the
    32 lane sums fold by the xor tree 16, 8, 4, 2, 1; lane 0's value)."""
    S = slabs.shape[0] if stop_after is None else stop_after
    if reducer == REDUCE_SERIAL:
        s = np.zeros(slabs.shape[1:], dtype=F32)
        for k in range(S):
            s = s + slabs[k]
        return s
    lanes = np.zeros((32,) + slabs.shape[1:], dtype=F32)
    for k in range(S):
        lanes[k % 32] = lanes[k % 32] + slabs[k]
    for o in (16, 8, 4, 2, 1):
        lanes = lanes + lanes[np.arange(32) ^ o]
    return lanes[0]


def wg_emul(c, dy, x, reducer=None, drop_last_split=False, stale_empty=False, drop_pixel_tail=False, drop_last_step=False):
    """ssg_gemm_wgrad_bf16 in float32: split z owns K-steps [z sps, (z + 1) sps) of 32 pixels, two 16-pixel MFMAs each into its fp32
    slab; then the ordered reduce (`reducer` overrides the one the host rule picks: both orders can be tried on one case).
    Defects: the last non-empty split never reduced; an empty split's slab holding stale data (the previous slab's) instead of zeros;
    pixel P - 1 dropped; the last K-step of every split dropped."""
    P, M, N = c.P, c.M, c.N
    S, sps = c.splits, c.sps
    tot = S * sps * 32
    d = np.zeros((tot, M), dtype=F64); d[:P] = dy
    v = np.zeros((tot, N), dtype=F64); v[:P] = x
    if drop_pixel_tail:
        d[P - 1] = 0
    d = d.reshape(S, sps * 2, 16, M); v = v.reshape(S, sps * 2, 16, N)
    slabs = np.zeros((S, M, N), dtype=F32)
    for h in range(2 * (sps - (1 if drop_last_step else 0))):
        slabs = _acc(slabs, np.matmul(d[:, h].transpose(0, 2, 1), v[:, h]))
    used = S - c.empty
    if stale_empty:
        for z in range(used, S):
            slabs[z] = slabs[z - 1]
    if drop_last_split:
        slabs[used - 1] = 0
    return wg_reduce_emul(slabs, reducer or c.reducer)


def _im2col(c, xr, swap_kykx=False, pad_wrong_side=False):
    """[N, OH, OW, taps, Cin] fp64: the input value each (output pixel, tap) meets.  Defects: tap (ky, kx) read at (kx, ky); the pad
    taken from the bottom / right (symmetric pads are unchanged, one-sided ones move the window)."""
    pt, pb, pl, pr = c.pads
    if pad_wrong_side:
        pt, pl = pb, pr
    cv = _canvas(xr, max(c.KH, c.KW), max(c.KH, c.KW), c.stride, pt, pl, c.OH, c.OW)
    cols = []
    for ky in range(c.KH):
        for kx in range(c.KW):
            a, b = (kx, ky) if swap_kykx else (ky, kx)
            cols.append(_tap(cv, a, b, c.stride, c.OH, c.OW))
    return np.stack(cols, axis=3)


def stem_fwd_emul(c, x, w, truncate=False, swap_kykx=False, pad_wrong_side=False, x_unrounded=False):
    """ssg_conv2d_thin_bf16 in float32: per output one fma chain over (ky, kx, c) in that order, fp32, then the bf16 store.  Products
    of two bf16 values are exact, so each fma is `accumulator + exact product` rounded once, which _acc reproduces: this emulation is
    bit-exact for the kernel's order.  A tap outside the image is skipped (adding nothing: the same bits)."""
    xr = (f32(x) if x_unrounded else bf16_rne(x)).astype(F64)
    wr = bf16_rne(w).astype(F64).reshape(c.Cout, c.Cin, c.KH * c.KW)
    col = _im2col(c, xr, swap_kykx, pad_wrong_side)
    acc = np.zeros((c.N, c.OH, c.OW, c.Cout), dtype=F32)
    for t in range(c.KH * c.KW):
        for ci in range(c.Cin):
            acc = _acc(acc, col[:, :, :, t, ci, None] * wr[None, None, None, :, ci, t])
    return bf16_trunc(acc) if truncate else bf16_rne(acc)


def stem_wgrad_emul(c, x, dy, wrap_early=False, stop_after_64=False, x_unrounded=False, swap_kykx=False, pad_wrong_side=False):
    """ssg_conv2d_thin_bf16_wgrad in float32: block b owns pixels [b per_block, (b + 1) per_block), lane q of WG_PL every WG_PL-th of
    them from b per_block + q on, fp32 fma per pixel; lane 0 adds the other lanes' sums in order; the blocks' partials are summed in
    fp64 and stored as fp32.  The lanes walk (n, oy, ox) incrementally as the kernel does.  Defects: the walk wrapping one pixel early
    at a row end (ox >= OW - 1 instead of ox >= OW); the reducer stopping after 64 blocks; x not rounded to bf16."""
    xr = (f32(x) if x_unrounded else bf16_rne(x)).astype(F64)
    col = _im2col(c, xr, swap_kykx, pad_wrong_side)                              # [N, OH, OW, T, Cin]
    d = np.asarray(dy, dtype=F64)
    P = c.N * c.OH * c.OW
    B, PB, L, T = c.blocks, c.per_block, c.wg_pl, c.KH * c.KW
    p = (np.arange(B) * PB)[:, None] + np.arange(L)[None, :]                      # [B, L]
    p1 = np.minimum((np.arange(B) + 1) * PB, P)[:, None]
    live = p < p1
    pc = np.minimum(p, P - 1)
    ox = pc % c.OW; oy = (pc // c.OW) % c.OH; n = pc // (c.OW * c.OH)
    acc = np.zeros((B, L, T, c.Cout, c.Cin), dtype=F32)
    d2 = d.reshape(P, c.Cout)
    while live.any():
        ok = live & (n < c.N)
        nn, yy, xx = np.where(ok, n, 0), np.where(ok, oy, 0), np.where(ok, ox, 0)
        g = d2[np.minimum(p, P - 1)] * live[..., None]                            # dy is addressed by p itself
        xv = col[nn, yy, xx] * ok[..., None, None]                                # [B, L, T, Cin]
        acc = _acc(acc, g[:, :, None, :, None] * xv[:, :, :, None, :])
        p = p + L
        live = p < p1
        ox = ox + L
        lim = c.OW - 1 if (wrap_early and c.OW > 1) else c.OW
        while True:
            over = ox >= lim
            if not over.any():
                break
            ox = np.where(over, ox - lim, ox)
            oy = np.where(over, oy + 1, oy)
            roll = oy >= c.OH
            oy = np.where(roll, 0, oy); n = np.where(roll, n + 1, n)
    part = acc[:, 0]
    for l in range(1, L):
        part = part + acc[:, l]
    nb = min(B, 64) if stop_after_64 else B
    s = part[:nb].astype(F64).sum(axis=0)                                         # [T, Cout, Cin]
    return np.ascontiguousarray(s.astype(F32).transpose(1, 2, 0)).reshape(c.Cout, c.Cin, c.KH, c.KW)


def stem_dgrad_emul(c, dy, w, ignore_parity=False, swap_kykx=False):
    """ssg_conv2d_thin_bf16_dgrad in float32: per input pixel one fma chain over (ky, kx, co) for the taps that reach it.  Defect: the
    stride parity test left out (oy = (iy + pad_t - ky) / stride taken whatever the remainder)."""
    d = np.asarray(dy, dtype=F64); wr = bf16_rne(w).astype(F64)
    pt, _, pl, _ = c.pads
    s = c.stride
    iy = np.arange(c.H)[:, None]; ix = np.arange(c.W)[None, :]
    acc = np.zeros((c.N, c.H, c.W, c.Cin), dtype=F32)
    for ky in range(c.KH):
        ty = iy + pt - ky
        oky = (ty >= 0) & ((ty % s == 0) | ignore_parity) & (ty // s < c.OH)
        for kx in range(c.KW):
            tx = ix + pl - kx
            ok = oky & (tx >= 0) & ((tx % s == 0) | ignore_parity) & (tx // s < c.OW)
            oy = np.broadcast_to(np.clip(ty // s, 0, c.OH - 1), ok.shape); ox = np.broadcast_to(np.clip(tx // s, 0, c.OW - 1), ok.shape)
            g = d[:, oy, ox] * ok[None, :, :, None]                               # [N, H, W, Cout]
            a, b = (kx, ky) if swap_kykx else (ky, kx)
            for co in range(c.Cout):
                acc = _acc(acc, g[..., co, None] * wr[co, :, a, b])
    return acc


# ============================================================================ coverage
# What each entry point accepts, from its SSG_REQUIRE lines, as facts some case must carry.
REQUIRED_FACTS = {
    'gemm': {'P=1', 'full_tile', 'tail8', 'tail16', 'tail24', 'nsteps1', 'nsteps2', 'nsteps3', 'nsteps4', 'nsteps5', 'ring_wrap', 'tiles<8', 'tiles7',
             'tiles8', 'tiles9', 'tiles19', 'tiles12', 'col_tiles2', 'col_tiles3', 'remap_full', 'remap_tail', 'ld_gaps', 'res_on_off', 'Kp+32',
             'nan_pack_rows', 'transpose', 'K=672'},
    'wgrad': {'P=1', 'P<32', 'P=32', 'P=33', 'ring_wrap', 'tiles2', 'tiles3', 'tiles6', 'splits2', 'empty_split', 'ragged_P', 'splits63', 'splits64',
              'reduce32', 'splits78', 'split_cap', 'ld_gaps'},
    'stem': {'pl1', 'pl2', 'pl3', 'pl4', 'k1', 'k1x3', 'k5', 'cin1', 'cin4', 'stride1', 'stride2', 'sym_pad', 'same_pad', 'pad1212', 'odd_hw', 'ow1',
             'ow2', 'ow3', 'wrap_loop', 'one_block', 'blocks2-64', 'blocks72', 'second_lap', 'block_cap', 'empty_block', 'items<256', 'items4096',
             'ragged_items'},
    'rows': {'C=4', 'C=8', 'C=12', 'C=40', 'odd_items', 'items<512', 'several_blocks'},
}
# Features the entry points accept that no case reaches, each with its reason.
LEFT_OUT = {
    'gemm: more than 2^31 / 128 pixel tiles': 'the grid-size refusal needs a tensor of 2^38 pixels; it is a host check, exercised by no launch',
    'gemm / wgrad: K, M, N above 672': 'the tile and step arithmetic does not change past three column tiles and 21 K-steps; tests/test_bf16_gpu.py keeps the workload shapes up to 2688',
    'wgrad: slabs above 64 KB and 512 KB (targets 1024 and 512) at the split cap': 'reached only with M N > 16384 and > 10^5 pixels: tens of seconds of host reference; p20000_112x672 takes the 1024 target below its cap',
    'stem: Cin = 2': 'the same zero-weight pad lanes as Cin = 1 and 3',
    'stem: windows with KH != KW other than 1 x 3': 'the tap decode is one division by KW, reached by 1 x 3, 3 x 3 and 5 x 5',
    'stem: ldx above 8': 'the pixel stride enters one multiplication; 4 and 8 are both used',
    'stem: more than 2^31 output pixels / 2^32 forward items': 'host refusals of tensors no test can hold',
    'pointers at a channel offset inside a wider row': 'the GEMMs take 16-byte aligned starts only; every buffer here starts a row, the gaps lie behind the valid channels',
    'rows: more than 2^31 items': 'the grid-stride loop of elem_grid; tests/test_layout_contract_gpu.py owns the large-index cases of pointwise.hip',
}


def check_coverage():
    """Every fact an entry point's table must reach is carried by a case; every case's literals agree with the restated host rules;
    every fact a case claims is a known one.  Returns the number of cases."""
    for t, need in REQUIRED_FACTS.items():
        have = set().union(*[c.facts for c in ALL_TABLES[t]])
        assert need <= have, (t, sorted(need - have))
        assert have <= need | {'one_split', 'per_block1024', 'ragged_blocks', 'nsteps21'}, (t, sorted(have - need))
    for c in GEMM_CASES:
        assert (c.tiles, c.nsteps) == gemm_plan(c.P, c.K, c.N)[:2], c.name
        assert c.K % 8 == 0 and c.N % 8 == 0 and c.Kp % 32 == 0 and c.Kp >= c.K, c.name
        for f, ok in (('tail8', c.K % 32 == 8), ('tail16', c.K % 32 == 16), ('tail24', c.K % 32 == 24), ('ring_wrap', c.nsteps >= 3),
                      ('tiles<8', c.tiles < 8), ('remap_full', c.tiles % 8 == 0), ('remap_tail', c.tiles > 8 and c.tiles % 8),
                      ('Kp+32', c.Kp == round_up(c.K, 32) + 32), ('transpose', c.transpose == 1), ('nan_pack_rows', c.nan_rows and c.N % 128)):
            assert f not in c.facts or ok, (c.name, f)
    assert {c.P for c in GEMM_CASES} >= {1, 127, 128, 129} and {c.K for c in GEMM_CASES} >= {8, 24, 32, 40, 64, 72, 96, 104, 136, 672}
    assert {c.N for c in GEMM_CASES} >= {8, 120, 128, 136, 264}
    for c in WG_CASES:
        assert (c.splits, c.sps, c.empty, c.reducer, c.ws_bytes) == wg_plan(c.P, c.M, c.N), (c.name, wg_plan(c.P, c.M, c.N))
        assert ('empty_split' in c.facts) == (c.empty > 0) and ('reduce32' in c.facts) == (c.reducer == REDUCE_32), c.name
    assert {c.P for c in WG_CASES} >= {1, 31, 32, 33, 255, 256, 512, 4133, 20000, 524320}
    assert {c.M for c in WG_CASES} | {c.N for c in WG_CASES} >= {8, 24, 128, 136, 264}
    for c in ALL_TABLES['stem']:
        pt, pb, pl, pr = c.pads
        assert c.OH == (c.H + pt + pb - c.KH) // c.stride + 1 and c.OW == (c.W + pl + pr - c.KW) // c.stride + 1, c.name
        assert (c.blocks, c.per_block, c.wg_pl, c.items, c.grid, c.ws_bytes) == stem_plan(c.N, c.OH, c.OW, c.Cout, c.KH, c.KW), (c.name, stem_plan(c.N, c.OH, c.OW, c.Cout, c.KH, c.KW))
        assert 1 <= c.Cin <= 4 and c.Cout % 8 == 0 and c.KH * c.KW <= 25 and c.stride in (1, 2) and c.KH * c.KW * (c.Cout // 8) <= 256, c.name
        assert 'pl%d' % c.wg_pl in c.facts or c.name in ('k1x3c8', 'ow1_s2', 'ow2_s2_same', 'items4096', 'b5_c48', 'b72_s2_same', 'b2048_k1', 'k1c8_cin1'), c.name
        P = c.N * c.OH * c.OW
        for f, ok in (('ow%d' % c.OW, c.OW <= 3), ('second_lap', c.blocks > 64), ('empty_block', (c.blocks - 1) * c.per_block >= P),
                      ('block_cap', cdiv(P, 1024) > STEM_MAX_BLOCKS), ('wrap_loop', c.OW < c.wg_pl)):
            assert (f in c.facts) == bool(ok), (c.name, f)
    assert {c.Cin for c in STEM_CASES} == {1, 3, 4}
    assert {(c.KH, c.Cout) for c in STEM_CASES if c.KH == c.KW} >= {(3, 8), (3, 32), (3, 48), (3, 64), (5, 40), (5, 56), (1, 8)}
    for c in ROWS_CASES:
        items = c.P * c.C // 4
        assert c.C % 4 == 0 and all(l % 4 == 0 and l >= c.C for l in c.lds) and len(set(c.lds)) == 3, c.name
        assert ('odd_items' in c.facts) == (items % 2 == 1) and ('items<512' in c.facts) == (items < 512) and ('several_blocks' in c.facts) == (items > 512), c.name
    return sum(len(v) for v in ALL_TABLES.values())


# RMS gate: where emul() is not run, and why.  Every emulation is vectorised over blocks, splits and pixels and takes at most 1.5 s
# (the input gradient of b72_s2_same), so none is left out.
EXEMPT = {}


# ============================================================================ verdicts (shared by the rehearsal and the GPU tests)
def judge(cls, got, ref, bf16_out, gate=None, emu=None):
    """{gate name: ratio}, pass <= 1.  Classes 0 (integers) and 1 (one product): `got` equals the exactly known result, rounded once
    to bf16 where the output is bf16, bit for bit ('bits': 0 or inf).  Class 2: the hard per-element gate, and the RMS gate where
    an emulation is given."""
    if cls in (0, 1):
        want = bf16_rne(f32(ref)) if bf16_out else f32(ref)
        return {'bits': 0.0 if first_mismatch(got, want) is None else float('inf')}
    out = {'hard': worst(got, ref, gate)}
    if emu is not None:
        out['rms'] = rms_ratio(got, emu, ref)
    return out


def passes(ratios):
    return all(v <= 1.0 for v in ratios.values())


def gemm_data(c, cls, variant=0):
    return (gemm_int_data, lambda c: gemm_onehot_data(c, variant), gemm_rand_data)[cls](c)


def wg_data(c, cls, variant=0):
    return (wg_int_data, lambda c: wg_onehot_data(c, variant), wg_rand_data)[cls](c)


def stem_data(c, cls, op, variant=0):
    return (stem_int_data, lambda c: stem_onehot_data(c, op, variant), stem_rand_data)[cls](c)


def res_buffer(c, res):
    """The residual as the kernels see it: [P][ldr = N + 16], NaN in the gap."""
    b = np.full((c.P, c.N + 16), np.nan, dtype=F32)
    b[:, :c.N] = res
    return b
