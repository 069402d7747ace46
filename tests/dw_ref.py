"""Plain references for csrc/depthwise.hip: the depthwise convolution (forward, input gradient, weight gradient; generic and
register-tiled kernels), the squeeze-excite plumbing (channel scale, per-sample channel sum, row broadcast) and the element-wise
ops (swish / sigmoid / gaussian, product), in fp32 and bf16.  Plain helper module in the style of bn_ref.py (not a conftest, no
fixtures), numpy only; nothing here calls an op under test.

Five kinds of thing:

* route / geometry -- dw_route, the part arithmetic of dwconv_wgrad_impl and sample_colsum_slices restated from the host code
                      (tests/test_dw_ref.py pins them to ssg_dwconv2d_kernel_id and the two workspace queries of the built library);
* *_ref            -- the operation in fp64, written from the formulas of include/ssunet_hip.h, each with its magnitude sum;
* gates            -- (rounding count) x (unit roundoff) x (magnitude sum) + one output rounding, each count derived beside it;
* case tables      -- the smallest shapes at which each kernel can still go wrong, and check_coverage(), which maps every case
                      through the restated route and asserts that every kernel id x op x dtype (and KW 3/5/7/9 on the tiled routes) is hit;
* *_emul           -- the tiled kernels' index arithmetic in fp32 (the 4-output thread and its v[] window, base / floor_half of the
                      stride-2 input gradient, the x-quad weight gradient with its parts, the slice sum), with the planted
                      defects of tests/test_dw_ref.py as keyword switches (all off).

No case is filtered by value and no gate holds a measured number."""
from collections import namedtuple
import functools

import numpy as np

from bn_ref import (DENORM, F32, F64, U32, U64, UBF, ULP32, bf16_rne, bf16_trunc, cdiv, f32, same_bits, sigmoid64,  # noqa: F401
                    sigmoid_emul, sigmoid_rel, swish_gate, swish_grad64, swish_grad_emul, swish_grad_gate, worst_ratio)

MIN_NORMAL = 2.0 ** -126
OP_FWD, OP_DGRAD, OP_WGRAD = 0, 1, 2
OPS = {'f': OP_FWD, 'd': OP_DGRAD, 'w': OP_WGRAD}
# ids of ssg_dwconv2d_kernel_id (include/ssunet_hip.h)
FWD_GENERIC, FWD_S1, FWD_S2 = 0, 1, 2
DGRAD_GENERIC, DGRAD_S1_FLIP, DGRAD_S2_EVEN, DGRAD_S2_ODD = 10, 11, 12, 13
WGRAD_GENERIC, WGRAD_S1, WGRAD_S2 = 20, 21, 22
IDS = {OP_FWD: (FWD_GENERIC, FWD_S1, FWD_S2), OP_DGRAD: (DGRAD_GENERIC, DGRAD_S1_FLIP, DGRAD_S2_EVEN, DGRAD_S2_ODD),
       OP_WGRAD: (WGRAD_GENERIC, WGRAD_S1, WGRAD_S2)}
TILED_IDS = (FWD_S1, FWD_S2, DGRAD_S1_FLIP, DGRAD_S2_EVEN, DGRAD_S2_ODD, WGRAD_S1, WGRAD_S2)
UNARY_SWISH, UNARY_SIGMOID, UNARY_GAUSSIAN = 0, 1, 2
DW_TQ, DW_PR, DW_XT = 16, 16, 4          # channel quads / pixel rows of a 256-thread reduction workgroup; outputs per thread


# ============================================================================ 1. route and geometry, restated from the host code
def route(op, stride, KH, KW, pl, NDH, C, aligned16):
    """dw_route of depthwise.hip.  NDH = N * rows of the tensor the call writes (grid.y of the tiled kernels)."""
    k35 = KW in (3, 5)
    k3579 = KW in (3, 5, 7, 9)
    if op == OP_WGRAD:
        return WGRAD_S1 if stride == 1 and k3579 else (WGRAD_S2 if stride == 2 and k35 else WGRAD_GENERIC)
    if op not in (OP_FWD, OP_DGRAD):
        return -1
    fits = bool(aligned16) and NDH <= 65535 and (C // 4 + 15) // 16 <= 65535
    s1 = fits and stride == 1 and k3579
    s2 = fits and stride == 2 and KH == KW and k35
    if op == OP_FWD:
        return FWD_S1 if s1 else (FWD_S2 if s2 else FWD_GENERIC)
    return DGRAD_S1_FLIP if s1 else ((DGRAD_S2_ODD if pl & 1 else DGRAD_S2_EVEN) if s2 else DGRAD_GENERIC)


WgradGeom = namedtuple('WgradGeom', 'tiled units parts rows_per_part chain')


def wgrad_geom(N, OH, OW, stride, KW):
    """The part arithmetic of dwconv_wgrad_impl.  Work units are pixels (generic) or x-quads of 4 consecutive output pixels
    (tiled); a workgroup's 16 pixel rows stride through a part's units, so one thread adds ceil(rows_per_part / 16) units, each of
    1 (generic) or 4 (tiled: the 4 pixels of an x-quad) products, into one accumulator: `chain`."""
    tiled = route(OP_WGRAD, stride, 0, KW, 0, 0, 4, True) != WGRAD_GENERIC
    units = N * OH * cdiv(OW, 4) if tiled else N * OH * OW
    parts = max(min(cdiv(units, 256), 256), 1)
    rpp = cdiv(units, parts)
    parts = cdiv(units, rpp)
    return WgradGeom(tiled, units, parts, rpp, cdiv(rpp, DW_PR) * (4 if tiled else 1))


def wgrad_workspace_bytes(N, OH, OW, C, KH, KW):
    """ssg_dwconv2d_wgrad_workspace_bytes: sized for the pixel count, which bounds the x-quad count."""
    P = N * OH * OW
    return max(min(cdiv(P, 256), 256), 1) * KH * KW * C * 8


ColsumGeom = namedtuple('ColsumGeom', 'slices rows_per_slice chain by_blocks')


def colsum_geom(N, S, C):
    """sample_colsum_slices and the rows_per_slice of sample_channel_sum_impl.  by_blocks: 2048 / blocks, not S / 256, set the count."""
    blocks = cdiv(C // 4, DW_TQ) * N
    z0 = 2048 // blocks
    maxz = S // (16 * DW_PR)
    z = max(min(z0, maxz, 1024), 1)
    rps = cdiv(S, z)
    return ColsumGeom(z, rps, cdiv(rps, DW_PR), z0 < min(maxz, 1024) and z0 >= 1)


def colsum_workspace_bytes(N, S, C):
    return N * colsum_geom(N, S, C).slices * C * 8


def out_hw(H, W, KH, KW, stride, pads):
    pt, pb, pl, pr = pads
    return (H + pt + pb - KH) // stride + 1, (W + pl + pr - KW) // stride + 1


# ============================================================================ 2. fp64 references, each with its magnitude sum
def _padded(x, KH, KW, stride, pads, OH, OW):
    pt, _, pl, _ = pads
    N, H, W, C = x.shape
    HP, WP = max((OH - 1) * stride + KH, pt + H), max((OW - 1) * stride + KW, pl + W)
    xp = np.zeros((N, HP, WP, C), dtype=F64)
    xp[:, pt:pt + H, pl:pl + W] = x
    return xp


def _tap(xp, ky, kx, stride, OH, OW):
    return xp[:, ky:ky + (OH - 1) * stride + 1:stride, kx:kx + (OW - 1) * stride + 1:stride]


def fwd_ref(x, w, bias, stride, pads):
    """out[n,oy,ox,c] = bias[c] + sum_k x[n, oy s + ky - pt, ox s + kx - pl, c] w[c,ky,kx]; (out, mag = |bias| + sum |x w|)."""
    x = np.asarray(x, dtype=F64); w = np.asarray(w, dtype=F64)
    C, KH, KW = w.shape
    OH, OW = out_hw(x.shape[1], x.shape[2], KH, KW, stride, pads)
    xp = _padded(x, KH, KW, stride, pads, OH, OW)
    out = np.zeros((x.shape[0], OH, OW, C), dtype=F64)
    mag = np.zeros_like(out)
    if bias is not None:
        out += np.asarray(bias, dtype=F64); mag += np.abs(np.asarray(bias, dtype=F64))
    for ky in range(KH):
        for kx in range(KW):
            t = _tap(xp, ky, kx, stride, OH, OW) * w[:, ky, kx]
            out += t; mag += np.abs(t)
    return out, mag


def dgrad_ref(g, w, stride, pads, H, W):
    """dx[n,y,x,c] = sum over (ky,kx,oy,ox) with oy s + ky - pt == y, ox s + kx - pl == x of g[n,oy,ox,c] w[c,ky,kx]; (dx, mag)."""
    g = np.asarray(g, dtype=F64); w = np.asarray(w, dtype=F64)
    C, KH, KW = w.shape
    N, OH, OW, _ = g.shape
    pt, _, pl, _ = pads
    dxp = _padded(np.zeros((N, H, W, C)), KH, KW, stride, pads, OH, OW)
    magp = np.zeros_like(dxp)
    for ky in range(KH):
        for kx in range(KW):
            t = g * w[:, ky, kx]
            _tap(dxp, ky, kx, stride, OH, OW)[...] += t
            _tap(magp, ky, kx, stride, OH, OW)[...] += np.abs(t)
    return dxp[:, pt:pt + H, pl:pl + W].copy(), magp[:, pt:pt + H, pl:pl + W].copy()


def wgrad_ref(x, g, KH, KW, stride, pads):
    """dw[c,ky,kx] = sum_{n,oy,ox} g[n,oy,ox,c] x[n, oy s + ky - pt, ox s + kx - pl, c]; (dw, mag = sum |g x|).  The products
    of fp32 values are exact in fp64; they are added in long double and rounded once."""
    x = np.asarray(x, dtype=F64); g = np.asarray(g, dtype=F64)
    N, OH, OW, C = g.shape
    xp = _padded(x, KH, KW, stride, pads, OH, OW)
    dw = np.zeros((C, KH, KW), dtype=F64); mag = np.zeros_like(dw)
    for ky in range(KH):
        for kx in range(KW):
            t = (g * _tap(xp, ky, kx, stride, OH, OW)).reshape(-1, C)
            dw[:, ky, kx] = t.sum(axis=0, dtype=np.longdouble).astype(F64)
            mag[:, ky, kx] = np.abs(t).sum(axis=0, dtype=np.longdouble).astype(F64)
    return dw, mag


def channel_scale_ref(x, s):
    """y[n,p,c] = x[n,p,c] s[n,c]; x [N,S,C], s [N,C]."""
    return np.asarray(x, dtype=F64) * np.asarray(s, dtype=F64)[:, None, :]


def channel_sum_ref(a, b, scale):
    """out[n,c] = scale sum_p a[n,p,c] (b ? b[n,p,c] : 1); (out, mag = |scale| sum |a b|).  scale is the fp32 the kernel gets."""
    t = np.asarray(a, dtype=F64)
    if b is not None:
        t = t * np.asarray(b, dtype=F64)
    sc = float(F32(scale))
    return sc * t.sum(axis=1, dtype=np.longdouble).astype(F64), abs(sc) * np.abs(t).sum(axis=1, dtype=np.longdouble).astype(F64)


def broadcast_ref(s, scale, S):
    """y[n,p,c] = scale s[n,c]."""
    s = np.asarray(s, dtype=F64)
    return np.broadcast_to((float(F32(scale)) * s)[:, None, :], (s.shape[0], S, s.shape[1])).copy()


def unary_ref(z, op):
    """(y, dy/dz) in fp64 by the formulas of the header: swish z sigma(z) with the reference's s (1 + z (1 - s)), sigmoid,
    exp(-z^2).  At the infinities the formulas are taken as written (inf * 0 = NaN), as the fp32 kernels take them."""
    z = np.asarray(z, dtype=F64)
    with np.errstate(all='ignore'):
        if op == UNARY_GAUSSIAN:
            e = np.exp(-(z * z))
            return e, -2.0 * z * e
        s = sigmoid64(z)
        if op == UNARY_SIGMOID:
            return s, s * (1.0 - s)
        return z * s, s * (1.0 + z * (1.0 - s))


# ============================================================================ 3. gates
# Forward and input gradient (all six kernels): acc starts as the bias (exact) and takes `taps` = KH KW terms, each either an
# fma (one rounding of the new partial sum) or a rounded product and a rounded sum (u |x w| + u |partial|).  Every partial sum
# is bounded by mag = |bias| + sum |x w| (to first order), so the sums cost at most taps u mag and the products, when they
# round at all, sum u |x w| <= u mag: (taps + 1) u mag under either contraction.  One more u mag covers the second-order terms
# ((1 + u)^(taps + 1) - 1 - (taps + 1) u, taps <= 121).  Taps that fall in the padding add an exact zero; they are counted anyway.
def conv_gate(taps, mag, ref=None, bf16=False):
    g = (taps + 2) * U32 * np.asarray(mag, dtype=F64)
    if bf16:                                             # one round-to-nearest-even store of the fp32 result (st4): 2^-8 |value|
        g = g + UBF * np.abs(ref)
    return g


# Weight gradient, fp32 tensors: the products (24 x 24 bits) are exact in fp64; per-thread sums, the 16-row LDS combine, the
# lanes of the second stage and its xor tree are all fp64 sums of those exact terms, P of them in some fixed order: every one of
# the P - 1 additions rounds a partial sum bounded by mag, so the fp64 total is within P 2^-53 mag; the store rounds it once to fp32.
# bf16 tensors: the products (8 x 8 bits) are exact in fp32, and a thread adds its `chain` products (wgrad_geom) in fp32: chain
# roundings (one per addition, the first into an exact zero included), each of a partial sum bounded by the thread's share of mag;
# summed over the threads chain u32 mag.  The fp64 stages above it add P 2^-53 mag, covered by one more u32 mag; the store rounds once.
def wgrad_gate(ref, mag, P, chain, bf16=False):
    ref = np.abs(np.asarray(ref, dtype=F64)); mag = np.asarray(mag, dtype=F64)
    if bf16:
        return (chain + 1) * U32 * mag + U32 * ref
    return U32 * ref + P * U64 * mag


# Per-sample channel sum: the same two-stage reduction over the S pixels of a sample, S terms in fp64 (fp32 tensors) or `chain` =
# ceil(rows_per_slice / 16) fp32 additions per thread (bf16 tensors, colsum_geom).  The terms are a, exact, or a b: exact in fp32
# for bf16 operands (16 bits), one fp32 rounding each for fp32 operands (u32 sum |a b|).  The finishing kernel multiplies the fp64
# total by the fp32 scale in fp64 (2^-53, covered by the + 1 below) and rounds once to fp32.  mag and ref already hold |scale|.
def channel_sum_gate(ref, mag, S, chain, bf16=False, with_b=False):
    ref = np.abs(np.asarray(ref, dtype=F64)); mag = np.asarray(mag, dtype=F64)
    if bf16:
        return (chain + 1) * U32 * mag + U32 * ref
    return U32 * ref + (S + 1) * U64 * mag + (U32 * mag if with_b else 0.0)


def one_rounding_gate(ref, bf16=False):
    """Channel scale, row broadcast, product and its two gradients: one product of two stored values, rounded once.  fp32: u32 |ref|.
    bf16: the tests' gate values and scales are bf16-representable, so the fp32 product (8 x 8 bits) is exact and the store's
    round-to-nearest-even is the one rounding: 2^-8 |ref|."""
    return (UBF if bf16 else U32) * np.abs(np.asarray(ref, dtype=F64))


# Unary ops.  sigm(z) = 1 / (1 + expf(-z)): expf and the division are at least as accurate as the v_exp_f32 / v_rcp_f32 pair that
# bn_ref.sigmoid_rel counts (1 ulp each), so its relative bound and the swish gates built on it hold here as they stand.  Below
# z = -88.7 the intermediate e^-z exceeds FLT_MAX, so 1 / (1 + inf) = 0 stands for a sigma < 2^-128: every value of sigma that small,
# and any result in the subnormal range, is compared to within one smallest normal number (times the factor it is multiplied by).
def unary_gates(z, op, g=None):
    """(gate of y, gate of dx = g * d) at fp32 arguments z; g: the incoming gradient (default 1, no product rounding)."""
    z = np.nan_to_num(np.asarray(z, dtype=F64), nan=0.0, posinf=3.4e38, neginf=-3.4e38)     # the gates stay finite; infinite and
    with np.errstate(all='ignore'):                                                          # NaN results are compared by class
        y, d = unary_ref(z, op)
        az = np.abs(z)
        if op == UNARY_GAUSSIAN:
            # t = z z rounds (u32 z^2, amplified to a relative u32 z^2 by the exponential), the negation is exact, expf 1 ulp;
            # d = (-2 z) e: the doubling is exact, the product rounds once more.
            rel = az * az * U32 + ULP32
            gy = np.abs(y) * rel + MIN_NORMAL
            gd = np.abs(d) * (rel + U32) + MIN_NORMAL * (1 + 2 * az)
        elif op == UNARY_SIGMOID:
            # d = s (1 - s): ds (1 - s) + s (ds + u32 (1 - s)) + u32 s (1 - s), ds = s sigmoid_rel
            s = sigmoid64(z); ds = s * sigmoid_rel(z) + MIN_NORMAL
            gy = ds
            gd = ds * (1 - s) + s * (ds + U32 * (1 - s)) + U32 * s * (1 - s) + MIN_NORMAL
        else:
            gy = swish_gate(z, 0.0) + MIN_NORMAL * (1 + az)
            gd = swish_grad_gate(z, 0.0) + MIN_NORMAL * (1 + az)
        if g is not None:
            ag = np.abs(np.asarray(g, dtype=F64))
            gd = ag * gd + U32 * np.abs(ag * d)          # dx = g * d: d's error times |g|, and the product's rounding
    return gy, gd


def classes(a):
    """0 finite, 1 +inf, 2 -inf, 3 NaN."""
    a = np.asarray(a, dtype=F64)
    return np.where(np.isnan(a), 3, np.where(np.isposinf(a), 1, np.where(np.isneginf(a), 2, 0)))


def unary_ratio(got, ref, gate):
    """Worst |got - ref| / gate over the finite references, inf where the classes (finite / +inf / -inf / NaN) differ."""
    got = np.asarray(got, dtype=F64); ref = np.asarray(ref, dtype=F64)
    if not np.array_equal(classes(got), classes(ref)):
        return float('inf')
    fin = classes(ref) == 0
    return worst_ratio((got - ref)[fin], np.asarray(gate, dtype=F64)[fin])


# ============================================================================ 4. case tables
# (name, N, H, W, C, KH, KW, stride, (pt, pb, pl, pr), ops, lds, off).  ops: letters of f(wd) d(grad) w(grad).
# lds = (ld of x, of y, of dy, of dx) or None (dense); off = (fp32, bf16) channel offset of every tensor's slice in its wider rows.
DwCase = namedtuple('DwCase', 'name N H W C KH KW stride pads ops lds off')


def _c(name, N, H, W, C, K, stride, pads, ops='fdw', lds=None, off=(0, 0)):
    KH, KW = K if isinstance(K, tuple) else (K, K)
    pads = (pads,) * 4 if isinstance(pads, int) else tuple(pads)
    return DwCase(name, N, H, W, C, KH, KW, stride, pads, ops, lds, off)


LD_STRIDES = (56, 48, 64, 72)          # x, y, dy, dx of bn_ref.LD_CASE_STRIDES: all distinct, multiples of 8


def _dw_cases():
    cs = []
    # widths around the thread's 4 outputs and the workgroup's 64 columns.  Stride 1: OW = W for fwd, dgrad and wgrad alike.
    for W in (1, 2, 3, 5, 63, 64, 65, 67):
        cs.append(_c('w%d_s1k3' % W, 1, 3, W, 8, 3, 1, 1))
    # stride 2, "same" pads (0,1,0,1)
    # (even W) and symmetric 1 (odd W): OW over the same set either way (the input gradient's width is W, of both parities)
    for OW in (1, 2, 3, 5, 63, 64, 65, 67):
        cs.append(_c('ow%d_s2k3_even' % OW, 1, 4, 2 * OW, 8, 3, 2, (0, 1, 0, 1)))
        cs.append(_c('ow%d_s2k3_odd' % OW, 1, 4, 2 * OW - 1, 8, 3, 2, 1))
    for W in (63, 65, 67):
        cs.append(_c('w%d_s2k5' % W, 1, 5, W, 8, 5, 2, 2))
    # images narrower and shorter than the kernel
    cs += [_c('w1_k9', 2, 3, 1, 8, 9, 1, 4), _c('w2_k9', 2, 3, 2, 8, 9, 1, 4), _c('h1_k9', 2, 1, 7, 8, 9, 1, 4),
           _c('h1_k3', 2, 1, 5, 8, 3, 1, 1), _c('h1w1_s2k5', 2, 1, 1, 8, 5, 2, 2), _c('h2w2_s2k3', 2, 2, 2, 8, 3, 2, (0, 1, 0, 1))]
    # channels around the 16-quad block
    for C in (4, 8, 60, 64, 68, 132):
        cs.append(_c('c%d_s1k3' % C, 2, 5, 6, C, 3, 1, 1))
    for C in (4, 60, 68, 132):
        cs.append(_c('c%d_s2k5' % C, 2, 5, 6, C, 5, 2, (1, 2, 1, 2)))
    # stride 2: H, W odd and even, left pads 0, 1, 2 (both PLODD forms for k3 and k5)
    for (H, W) in ((7, 10), (8, 9)):
        for K in (3, 5):
            for pads in ((0, 1, 0, 1), (1, 2, 1, 2), 1, 2, (0, 0, 0, 0)):
                p = (pads,) * 4 if isinstance(pads, int) else pads
                cs.append(_c('s2k%d_%dx%d_p%d%d%d%d' % ((K, H, W) + p), 2, H, W, 8, K, 2, pads))
    # stride 1: pads (0,2,0,2) and K // 2
    for K in (3, 5, 7, 9):
        cs.append(_c('s1k%d_p0202' % K, 2, 9, 11, 8, K, 1, (0, 2, 0, 2)))
        cs.append(_c('s1k%d_same' % K, 2, 9, 11, 8, K, 1, K // 2))
    # rectangular kernels (the tiled routes look at KW alone at stride 1; at stride 2 only the weight gradient stays tiled)
    for (KH, KW) in ((3, 5), (5, 3), (7, 1), (1, 7)):
        cs.append(_c('rect%dx%d_s1' % (KH, KW), 2, 8, 10, 8, (KH, KW), 1, (KH // 2, KH // 2, KW // 2, KW // 2)))
    for (KH, KW) in ((3, 5), (5, 3)):
        cs.append(_c('rect%dx%d_s2' % (KH, KW), 2, 8, 11, 8, (KH, KW), 2, (KH // 2, KH // 2, KW // 2, KW // 2)))
    # sizes that must fall to the generic kernels
    cs += [_c('k2', 2, 6, 7, 8, 2, 1, (0, 1, 0, 1)), _c('k4', 2, 6, 7, 8, 4, 1, (1, 2, 1, 2)), _c('k11', 2, 6, 7, 8, 11, 1, 5),
           _c('s3k3', 2, 8, 10, 8, 3, 3, 1), _c('s2k7', 2, 9, 10, 8, 7, 2, 3), _c('s4k5', 2, 9, 11, 8, 5, 4, 2)]
    # the grid limit from both sides: N * H = 65535 stays tiled, 65792 falls back (forward and input gradient; OH = H)
    cs += [_c('grid_n255', 255, 257, 3, 4, 3, 1, 1, ops='fd'), _c('grid_n256', 256, 257, 3, 4, 3, 1, 1, ops='fd')]
    # weight gradient: one part; a ragged last part; work units above 65536 (parts capped at 256), tiled and generic
    cs += [_c('wg_onepart', 2, 13, 21, 8, 3, 1, 1, ops='w'), _c('wg_ragged_s1', 3, 17, 25, 8, 5, 1, 2, ops='w'),
           _c('wg_ragged_s2', 3, 35, 50, 8, 3, 2, (0, 1, 0, 1), ops='w'), _c('wg_ragged_gen', 3, 11, 13, 8, 4, 1, (1, 2, 1, 2), ops='w'),
           _c('wg_capped', 4, 130, 516, 4, 3, 1, 1, ops='w'), _c('wg_capped_gen', 4, 130, 130, 4, 2, 1, 0, ops='w')]
    # ld > C on every tensor with distinct strides; the slice starts 4 (fp32) / 8 (bf16) channels into its rows: 16-byte aligned
    cs += [_c('ld_s1k3', 2, 7, 9, 40, 3, 1, 1, lds=LD_STRIDES, off=(4, 8)), _c('ld_s2k5', 2, 7, 9, 40, 5, 2, (1, 2, 1, 2), lds=LD_STRIDES, off=(4, 8)),
           _c('ld_k4', 2, 7, 9, 40, 4, 1, (1, 2, 1, 2), lds=LD_STRIDES, off=(4, 8))]
    return cs


DW_CASES = _dw_cases()
# bf16 only: a slice that starts 4 channels into wider rows is 8-byte aligned, so forward and input gradient leave the tiled kernels
DW_CASES_BF16_UNALIGNED = [_c('slice4_s1k3', 2, 6, 9, 8, 3, 1, 1, lds=(16, 16, 16, 16), off=(0, 4)),
                           _c('slice4_s2k5', 2, 6, 9, 8, 5, 2, (1, 2, 1, 2), lds=(16, 16, 16, 16), off=(0, 4))]


def dw_cases(bf16):
    return DW_CASES + (DW_CASES_BF16_UNALIGNED if bf16 else [])


def case_aligned(case, bf16):
    return (case.off[1] * 2 if bf16 else case.off[0] * 4) % 16 == 0


def case_route(case, op, bf16):
    OH, OW = out_hw(case.H, case.W, case.KH, case.KW, case.stride, case.pads)
    ndh = case.N * (OH if op == OP_FWD else case.H)
    return route(op, case.stride, case.KH, case.KW, case.pads[2], ndh, case.C, case_aligned(case, bf16))


def check_coverage():
    """Every kernel id of every op is reached in each dtype, KW 3/5/7/9 (3/5 at stride 2) on every tiled route, and the weight
    gradient's part arithmetic at each of its edges.  Returns {(bf16, id): set of KW}."""
    hit = {}
    facts = set()
    for bf16 in (False, True):
        for case in dw_cases(bf16):
            OH, OW = out_hw(case.H, case.W, case.KH, case.KW, case.stride, case.pads)
            assert OH >= 1 and OW >= 1, case.name
            for o in case.ops:
                hit.setdefault((bf16, case_route(case, OPS[o], bf16)), set()).add(case.KW)
                if o == 'w':
                    g = wgrad_geom(case.N, OH, OW, case.stride, case.KW)
                    facts.add(('one_part', g.tiled) if g.parts == 1 else ('ragged', g.tiled) if g.units % g.rows_per_part else ('even', g.tiled))
                    if g.units > 65536:
                        assert g.parts == 256
                        facts.add(('capped', g.tiled))
                    if g.tiled:
                        facts.add(('ow%4', OW % 4))
    for bf16 in (False, True):
        for op, ids in IDS.items():
            for i in ids:
                assert (bf16, i) in hit, 'no %s case reaches kernel id %d' % ('bf16' if bf16 else 'fp32', i)
        for i in (FWD_S1, DGRAD_S1_FLIP, WGRAD_S1):
            assert hit[(bf16, i)] >= {3, 5, 7, 9}, (bf16, i, hit[(bf16, i)])
        for i in (FWD_S2, DGRAD_S2_EVEN, DGRAD_S2_ODD, WGRAD_S2):
            assert hit[(bf16, i)] >= {3, 5}, (bf16, i, hit[(bf16, i)])
    need = {('one_part', True), ('ragged', True), ('ragged', False), ('capped', True), ('capped', False)} | {('ow%4', r) for r in (1, 2, 3)}
    assert need <= facts, need - facts
    assert any(case_route(c, OP_FWD, True) == FWD_GENERIC and route(OP_FWD, c.stride, c.KH, c.KW, c.pads[2], 1, c.C, True) != FWD_GENERIC
               for c in DW_CASES_BF16_UNALIGNED), 'the 8-byte-aligned bf16 slice must leave a tiled route'
    return hit


# channel sums: (N, S, C); every case runs with b == NULL (scale 1 / S) and with b given (scale 0.75)
COLSUM_CASES = [(N, S, C) for S in (1, 255, 256, 511, 4096, 4097) for (N, C) in ((2, 8), (3, 132))] + [(16, 1024, 2688)]
COLSUM_LD = (3, 511, 40, 56, 64)       # (N, S, C, ld of a, ld of b): slices of wider rows
SE_CASES = [(2, 1, 8), (3, 255, 132), (2, 4097, 4), (3, 67, 60)]          # channel scale and row broadcast: (N, S, C)
UNARY_CASES = [(37, 8, 8, 8), (37, 132, 132, 132), (19, 40, 56, 48)]      # (P, C, ld of x / dy, ld of y / dx)
UNARY_PAD_CASE = (23, 6, 8, 8)         # the forward alone takes C % 4 != 0 and writes the pad lanes as 0
Z_SWEEP = [s * v for v in (0.0, 1e-30, 1.0, 20.0, 88.0, 89.0, 104.0, 1e4, float('inf')) for s in (1.0, -1.0)] + [float('nan')]


def check_colsum_coverage():
    geoms = [colsum_geom(*c) for c in COLSUM_CASES]
    assert any(g.slices == 1 for g in geoms) and any(g.slices > 1 and not g.by_blocks for g in geoms)
    assert colsum_geom(16, 1024, 2688).by_blocks and colsum_geom(16, 1024, 2688).slices == 3
    assert any(S % g.rows_per_slice for (N, S, C), g in zip(COLSUM_CASES, geoms) if g.slices > 1), 'a ragged last slice'


# ============================================================================ 5. data: seeded, nonzero means, bf16-representable for bf16
def _q(a, bf16):
    a = f32(a)
    return bf16_rne(a) if bf16 else a


def dw_data(case, bf16, seed=7):
    """(x [N,H,W,C], w [C,KH,KW], bias [C], g [N,OH,OW,C]) fp32 (bf16 cases: every value bf16-representable, weights included)."""
    rng = np.random.RandomState(seed + case.N * 131 + case.H * 17 + case.W * 3 + case.C + case.KW * 7 + case.stride)
    OH, OW = out_hw(case.H, case.W, case.KH, case.KW, case.stride, case.pads)
    x = _q(0.5 + rng.standard_normal((case.N, case.H, case.W, case.C)), bf16)
    w = _q(0.2 + 0.5 * rng.standard_normal((case.C, case.KH, case.KW)), bf16)
    b = _q(rng.standard_normal(case.C), bf16)
    g = _q(-0.3 + rng.standard_normal((case.N, OH, OW, case.C)), bf16)
    return x, w, b, g


@functools.lru_cache(maxsize=2)
def colsum_data(N, S, C, bf16, seed=11):
    rng = np.random.RandomState(seed + N + S + C)
    a = _q(0.25 + rng.standard_normal((N, S, C)).astype(F32), bf16)
    b = _q(-0.5 + rng.standard_normal((N, S, C)).astype(F32), bf16)
    a.setflags(write=False); b.setflags(write=False)
    return a, b


def se_data(N, S, C, bf16, seed=13):
    rng = np.random.RandomState(seed + N + S + C)
    return _q(0.5 + rng.standard_normal((N, S, C)), bf16), _q(rng.uniform(0.05, 1.0, (N, C)), bf16)


def unary_data(P, C, seed=17):
    """x [P, C] around 0.3 with std 3, its first entries the sweep of extreme arguments; g [P, C]."""
    rng = np.random.RandomState(seed + P + C)
    x = f32(0.3 + 3 * rng.standard_normal((P, C)))
    flat = x.reshape(-1)
    n = min(len(Z_SWEEP), flat.size)
    flat[:n] = f32(Z_SWEEP)[:n]
    return x, f32(0.7 + rng.standard_normal((P, C)))


# ============================================================================ 6. fp32 emulations of the tiled kernels
def _store(acc, bf16, truncate=False):
    acc = f32(acc)
    if not bf16:
        return acc
    return bf16_trunc(acc) if truncate else bf16_rne(acc)


def _gather_cols(rowsrc, ix, SW):
    """rowsrc [N, R, SW, C], ix [G]: columns ix with zeros outside [0, SW) -> [N, R, G, C] (the `v[]` loads of a thread)."""
    ok = (ix >= 0) & (ix < SW)
    v = rowsrc[:, :, np.clip(ix, 0, SW - 1), :]
    return np.where(ok[None, None, :, None], v, F32(0))


def s1_emul(src, w, bias, DH, DW, pt, pl, S=1, flip=False, bf16=False, drop_last_col=False, pad_off=False, bias_omit=False,
            bias_twice=False, truncate=False):
    """dw_s1_kernel<KW, T, S>: thread (xg, cq) of row (n, oy) owns outputs x0 .. x0 + 3, x0 = 4 * (column group); per kernel row it
    loads the NV = 3 S + KW source columns x0 S + j - pl once into v[] and applies tap kx to v[j S + kx].  Unwritten outputs stay
    NaN.  Defects: the store guard off by one when DW % 4 != 0, left pad off by one, bias left out / added twice, truncating store.
    `flip` off for the stride-1 input gradient is the not-flipped defect (the caller passes it)."""
    src = f32(src); w = f32(w)
    N, SH, SW, C = src.shape
    KH, KW = w.shape[1:]
    KK = KH * KW
    wf = w.reshape(C, KK)
    G = cdiv(DW, DW_XT)
    x0 = np.arange(G) * DW_XT
    if pad_off:
        pl = pl + 1
    b0 = np.zeros(C, dtype=F32) if (bias is None or bias_omit) else f32(bias) * F32(2 if bias_twice else 1)
    acc = np.broadcast_to(b0, (DW_XT, N, DH, G, C)).copy()
    oy = np.arange(DH)
    for ky in range(KH):
        iy = oy * S + ky - pt
        rok = (iy >= 0) & (iy < SH)
        rows = np.where(rok[None, :, None, None], src[:, np.clip(iy, 0, SH - 1)], F32(0))       # skipped rows add exact zeros
        NV = (DW_XT - 1) * S + KW
        v = [_gather_cols(rows, x0 * S + j - pl, SW) for j in range(NV)]
        for kx in range(KW):
            t = ky * KW + kx
            wv = wf[:, KK - 1 - t if flip else t]
            for j in range(DW_XT):
                acc[j] = acc[j] + v[j * S + kx] * wv
    out = np.full((N, DH, G * DW_XT, C), np.nan, dtype=F32)
    for j in range(DW_XT):
        out[:, :, x0 + j] = _store(acc[j], bf16, truncate)
    out = out[:, :, :DW].copy()
    if drop_last_col and DW % DW_XT:
        out[:, :, DW - 1] = np.nan
    return out


def _floor_half(t):
    return (t - (t & 1)) // 2


def dgrad_s2_emul(g, w, H, W, pt, pl, bf16=False, plodd_inverted=False, drop_last_col=False, pad_off=False, truncate=False):
    """dw_dgrad_s2_kernel<KW, T, PLODD>: thread owns dx columns x0 .. x0 + 3 (x0 % 4 == 0); per kernel row of matching parity it
    loads the NV = (4 + KW) / 2 + 1 dout columns from base = floor((x0 + pl - (KW - 1)) / 2) and applies tap kx to output j where
    e = j + PLODD - kx is even, from v[floor_half(e) - floor_half(PLODD - (KW - 1))].  Defects: PLODD inverted (the dispatch's
    `odd` test), store guard, left pad off by one, truncating store."""
    g = f32(g); w = f32(w)
    N, SH, SW, C = g.shape
    KH, KW = w.shape[1:]
    if pad_off:
        pl = pl + 1
    plodd = (pl & 1) ^ (1 if plodd_inverted else 0)
    G = cdiv(W, DW_XT)
    x0 = np.arange(G) * DW_XT
    t0 = x0 + pl - (KW - 1)
    base = (t0 - (t0 & 1)) // 2
    NV = (DW_XT + KW) // 2 + 1
    acc = np.zeros((DW_XT, N, H, G, C), dtype=F32)
    y = np.arange(H)
    for ky in range(KH):
        ty = y + pt - ky
        oy = ty >> 1
        rok = (ty >= 0) & ((ty & 1) == 0) & (oy < SH)
        rows = np.where(rok[None, :, None, None], g[:, np.clip(oy, 0, SH - 1)], F32(0))
        v = [_gather_cols(rows, base + q, SW) for q in range(NV)]
        for kx in range(KW):
            wv = w[:, ky, kx]
            for j in range(DW_XT):
                e = j + plodd - kx
                if (e & 1) == 0:
                    acc[j] = acc[j] + v[_floor_half(e) - _floor_half(plodd - (KW - 1))] * wv
    out = np.full((N, H, G * DW_XT, C), np.nan, dtype=F32)
    for j in range(DW_XT):
        out[:, :, x0 + j] = _store(acc[j], bf16, truncate)
    out = out[:, :, :W].copy()
    if drop_last_col and W % DW_XT:
        out[:, :, W - 1] = np.nan
    return out


def _fold32(lanes):
    """fold32: v += shfl_xor(v, o) for o = 16 .. 1 over axis 0 (32 lanes); every lane ends with the total, lane 0 is stored."""
    idx = np.arange(32)
    for o in (16, 8, 4, 2, 1):
        lanes = lanes + lanes[idx ^ o]
    return lanes[0]


def _second_stage(part):
    """dw_wgrad_final_kernel / sample_colsum_final_kernel: lane k adds partial rows k, k + 32, ... in row order, fold32.  part [rows, ...] fp64."""
    lanes = np.zeros((32,) + part.shape[1:], dtype=F64)
    for b in range(part.shape[0]):
        lanes[b % 32] = lanes[b % 32] + part[b]
    return _fold32(lanes)


def wgrad_tiled_emul(x, g, KH, KW, stride, pt, pl, bf16=False, drop_last_quad=False, drop_last_part=False, pad_off=False):
    """dw_wgrad_s1_kernel<KW, T, S> + dw_wgrad_final_kernel: kernel row ky per workgroup, units = x-quads of 4 output pixels, part b
    takes units [b rpp, min((b + 1) rpp, U)), pixel row pr of the workgroup the units u0 + pr, u0 + pr + 16, ...; per unit the 4 dout
    quads and the 3 S + KW input columns ox0 S + q - pl, s[kx] += g[j] v[j S + kx] over j in acc_t (fp64 for fp32 tensors, fp32 for
    bf16); 16-row combine and the second stage in fp64.  Defects: the last x-quad of every part / the last part left out; left pad."""
    x = f32(x); g = f32(g)
    N, H, W, C = x.shape
    _, OH, OW, _ = g.shape
    S = stride
    acc_t = F32 if bf16 else F64
    geo = wgrad_geom(N, OH, OW, S, KW)
    assert geo.tiled
    if pad_off:
        pl = pl + 1
    OW4 = cdiv(OW, 4)
    U, parts, rpp = geo.units, geo.parts, geo.rows_per_part
    u0 = np.arange(parts)[:, None] * rpp
    u1 = np.minimum(u0 + rpp, U) - (1 if drop_last_quad else 0)
    NV = 3 * S + KW
    xz = np.concatenate([x.reshape(-1, C), np.zeros((1, C), dtype=F32)])         # row -1: the zero a masked load returns
    gz = np.concatenate([g.reshape(-1, C), np.zeros((1, C), dtype=F32)])
    dw = np.zeros((C, KH, KW), dtype=F32)
    for ky in range(KH):
        s = np.zeros((KW, parts, DW_PR, C), dtype=acc_t)
        for i in range(cdiv(rpp, DW_PR)):
            u = u0 + np.arange(DW_PR)[None, :] + DW_PR * i                       # [parts, 16]
            live = u < u1
            uc = np.where(live, u, 0)
            xq = uc % OW4; r = uc // OW4
            oy = r % OH; n = r // OH
            iy = oy * S + ky - pt
            live = live & (iy >= 0) & (iy < H)
            ox0 = xq * 4
            gj = []
            for j in range(4):
                ok = live & (ox0 + j < OW)
                gj.append(gz[np.where(ok, (n * OH + oy) * OW + ox0 + j, -1)].astype(acc_t))
            vq = []
            for q in range(NV):
                ix = ox0 * S + q - pl
                ok = live & (ix >= 0) & (ix < W)
                vq.append(xz[np.where(ok, (n * H + iy) * W + ix, -1)].astype(acc_t))
            for kx in range(KW):
                for j in range(4):
                    s[kx] = s[kx] + gj[j] * vq[j * S + kx]
        for kx in range(KW):
            red = s[kx].astype(F64)
            tot = np.zeros((parts, C), dtype=F64)
            for r_ in range(DW_PR):
                tot = tot + red[:, r_]
            if drop_last_part and parts > 1:
                tot = tot[:-1]
            dw[:, ky, kx] = _second_stage(tot).astype(F32)
    return dw


def colsum_emul(a, b, scale, bf16=False, drop_last_slice=False, scale_per_slice=False):
    """sample_colsum_kernel + sample_colsum_final_kernel: slice z takes rows [z rps, min((z + 1) rps, S)), pixel row pr of the
    workgroup the rows p0 + pr, p0 + pr + 16, ... in acc_t (fp64 / fp32), a * b an fp32 product; 16-row combine, the slices added
    lane-then-row and folded in fp64, (float)(t * scale).  Defects: the last slice left out; the scale applied inside the slice loop."""
    a = f32(a)
    N, S, C = a.shape
    acc_t = F32 if bf16 else F64
    geo = colsum_geom(N, S, C)
    z, rps = geo.slices, geo.rows_per_slice
    v = a if b is None else a * f32(b)
    vz = np.concatenate([v, np.zeros((N, 1, C), dtype=F32)], axis=1)
    p0 = np.arange(z)[:, None] * rps
    p1 = np.minimum(p0 + rps, S)
    s = np.zeros((N, z, DW_PR, C), dtype=acc_t)
    for i in range(cdiv(rps, DW_PR)):
        p = p0 + np.arange(DW_PR)[None, :] + DW_PR * i
        s = s + vz[:, np.where(p < p1, p, S)].astype(acc_t)
    red = s.astype(F64)
    tot = np.zeros((N, z, C), dtype=F64)
    for r_ in range(DW_PR):
        tot = tot + red[:, :, r_]
    part = np.moveaxis(tot, 1, 0)                                                # [z, N, C]
    if drop_last_slice and z > 1:
        part = part[:-1]
    sc = float(F32(scale))
    if scale_per_slice:
        t = np.zeros(part.shape[1:], dtype=F64)
        for k in range(part.shape[0]):
            t = (t + part[k]) * sc
        return t.astype(F32)
    return (_second_stage(part) * sc).astype(F32)


def unary_emul(z, op, g=None):
    """unary_fwd_kernel / unary_bwd_kernel in fp32: (y, g * d)."""
    z = f32(z)
    with np.errstate(all='ignore'):
        if op == UNARY_GAUSSIAN:
            e = np.exp(-(z * z).astype(F64)).astype(F32)        # expf as a rounding of the exact value (numpy's fp32 exp errs by > 1 ulp)
            y, d = e, F32(-2) * z * e
        elif op == UNARY_SIGMOID:
            s = sigmoid_emul(z)
            y, d = s, s * (F32(1) - s)
        else:
            y, d = z * sigmoid_emul(z), swish_grad_emul(z)
        return f32(y), f32(d if g is None else f32(g) * d)


# ============================================================================ 7. comparisons shared by the rehearsal and the GPU file
def conv_ratio(got, ref, mag, taps, bf16):
    return worst_ratio(np.asarray(got, dtype=F64) - ref, conv_gate(taps, mag, ref, bf16))


def wgrad_ratio(got, ref, mag, case, bf16):
    OH, OW = out_hw(case.H, case.W, case.KH, case.KW, case.stride, case.pads)
    geo = wgrad_geom(case.N, OH, OW, case.stride, case.KW)
    return worst_ratio(np.asarray(got, dtype=F64) - ref, wgrad_gate(ref, mag, case.N * OH * OW, geo.chain, bf16))


def colsum_ratio(got, ref, mag, N, S, C, bf16, with_b):
    return worst_ratio(np.asarray(got, dtype=F64) - ref, channel_sum_gate(ref, mag, S, colsum_geom(N, S, C).chain, bf16, with_b))
