"""Plain references for ssg_conv2d_wgrad_f32 (csrc/conv_wgrad*.hip) and ssg_linear_wgrad_f32: the dense convolution's weight
gradient on every kernel route.  Plain helper module in the style of dw_ref.py (not a conftest, no fixtures), numpy only; nothing
here calls an op under test.

* route       -- make_plan, ssg_wgrad4_kind / _slices, ssg_wgrad_halo_ok, ssg_wgrad_k32_ok / _steps restated from the host code
                 (tests/test_wgrad_ref.py pins the restatement to ssg_conv2d_wgrad_kernel_id and the workspace query of the built
                 library at every case);
* wgrad_ref   -- the operation in fp64, written from the contract of include/ssunet_hip.h, with its magnitude sum;
* data        -- three classes: (a) integer-valued operands (every product and partial sum exact: bit-exact gate), (b) one non-zero
                 dout pixel (every element a single product: per-product accuracy of the bf16x3 split), (c) random full-mantissa
                 operands (accumulation: a hard per-element gate and an RMS gate against emul());
* gates       -- derived beside each;
* case table  -- the smallest shapes at which each route can still go wrong, and check_coverage();
* emul        -- the reduction in numpy float32 with the kernels' slab partition (a reference for the RMS gate, checked against
                 fp64 by the rehearsal), with the planted defects of tests/test_wgrad_ref.py as keyword switches (all off).

Kernel ids (ssg_conv2d_wgrad_kernel_id).  Reachable: 2 wgrad_kernel<128,32>; 20 / 21 wgrad_dma<128,128> / <128,64>; 50 / 51 their
split-operand (x3) forms; 30 / 31 wgrad_halo<32,128> / <64,64>; 40 / 41 wgrad_halo_x3; 60 wgrad_k32; 15 / 16 wgrad4 (4x4x1 MFMA,
thin dout / thin in); 17 wgrad_tiny4 (VALU); 18 wgrad32_cin (32x32x2 MFMA).  Listed by earlier headers but never returned:
0 and 1 -- make_plan gives variant 0 (Cout > 64) and 1 (32 < Cout <= 64) to the DMA or halo kernels always (wgrad_uses_dma is
variant <= 1), only variant 2 stays on the register-staged kernel; 13 and 14 -- a wgrad4 plan returns 10 + kind and
ssg_wgrad4_kind returns 0 or 5..8, so the smallest such id is 15.

No case is filtered by value and no gate holds a measured number."""
from collections import namedtuple

import numpy as np

from bn_ref import ACT_LRELU, ACT_NONE, ACT_RELU, F32, F64, U32, bf16_rne, cdiv, f32, preact_emul, same_bits, worst_ratio  # noqa: F401

REACHABLE_IDS = (2, 15, 16, 17, 18, 20, 21, 30, 31, 40, 41, 50, 51, 60)
UNREACHABLE_IDS = (0, 1, 13, 14)
SPLIT_IDS = (40, 41, 50, 51, 60)               # both operands as three bf16 terms, six products (mfma_split.h)
STRIP_IDS = {30: 16, 31: 16, 40: 16, 41: 16, 60: 32}      # K-step = KPX pixels of one row of a KPX-wide column strip
BKP, KP32, SEG, TINY_PIX = 16, 32, 32, 4096
LRELU_SLOPE = 0.25
FLT_MAX = float(np.finfo(np.float32).max)


# ============================================================================ 1. the case type and its geometry
# k: 3 (pad 1) or 1 (pad 0), taps row-major; flags: ssg_wgrad_desc.flags; k32: ssg_wgrad_set_k32_mode; cin_real: None = C1 + C2;
# ld1 / ld2 / ldd: None = dense (pad4 of the channels); aff: None or the in_act of a fused input transform;
# irange: the integers of class (a) lie in [-irange, irange]; stat: the case also runs class (b) and the RMS gate of class (c).
WgCase = namedtuple('WgCase', 'name N H W C1 C2 Cout k stride flags k32 cin_real ld1 ld2 ldd aff irange stat')
Geom = namedtuple('Geom', 'pad GH GW ntaps dy dx ky kx Cin cin_real ld1 ld2 ldd P')


def pad4(c):
    return (c + 3) // 4 * 4


def geom(c):
    p = c.k // 2
    GH, GW = (c.H + 2 * p - c.k) // c.stride + 1, (c.W + 2 * p - c.k) // c.stride + 1
    ky = [t // c.k for t in range(c.k * c.k)]; kx = [t % c.k for t in range(c.k * c.k)]
    Cin = c.C1 + c.C2
    return Geom(p, GH, GW, c.k * c.k, [y - p for y in ky], [x - p for x in kx], ky, kx, Cin, c.cin_real or Cin,
                c.ld1 or c.C1, c.ld2 or c.C2, c.ldd or pad4(c.Cout), c.N * GH * GW)


# ============================================================================ 2. make_plan, restated
Plan = namedtuple('Plan', 'kid kind variant mt nt steps sps splits zl aff_ok')


def wgrad4_kind(c, g):
    """ssg_wgrad4_kind: one input, unit stride over the whole image (3x3 pad 1 or 1x1 pad 0 here), 32-bit byte offsets."""
    if c.C2 or c.stride != 1 or g.GH != c.H or g.GW != c.W:
        return 0
    if c.N * c.H * c.W * max(g.ld1, g.ldd) >= 1 << 30:
        return 0
    if c.Cout <= 4 and c.C1 >= 16:
        return 5
    if c.C1 == 4 and c.Cout <= 8 and g.ntaps == 9:
        return 7
    if c.C1 == 4 and g.ntaps == 9 and c.Cout >= 32 and c.N * c.H * c.W >= 65536:
        return 8
    return 6 if c.C1 == 4 else 0


W4Slices = namedtuple('W4Slices', 'slabs groups upz spr waves')


def wgrad4_slices(c, kind):
    """ssg_wgrad4_slices: kind 7 one slab per 4096 pixels; else 32-pixel row segments dealt to ~8192 / groups waves, 4 waves a slab."""
    if kind == 7:
        return W4Slices(cdiv(c.N * c.H * c.W, TINY_PIX), 1, TINY_PIX, 1, 0)
    groups = cdiv(c.C1 if kind == 5 else c.Cout, 64)
    spr = cdiv(c.W, SEG)
    units = c.N * c.H * spr
    nz = max(min(8192 // groups, units), 1)
    upz = cdiv(units, nz)
    nz = cdiv(units, upz)
    return W4Slices(cdiv(nz, 4), groups, upz, spr, nz)


def halo_ok(c, g, variant):
    cb = 32 if variant == 0 else 64
    return c.k == 3 and c.stride == 1 and c.C1 % cb == 0 and c.C2 % cb == 0


def k32_ok(c, g):
    return bool(c.k32 and (c.flags & 1) and c.k == 3 and c.stride == 1 and c.C1 % 64 == 0 and c.C2 % 64 == 0 and c.Cout % 64 == 0
                and g.GW >= 17 and c.N * c.H * c.W * max(g.ld1, g.ld2) * 4 <= 0xfffffff0 and g.P * g.ldd * 4 <= 0xfffffff0)


def make_plan(c):
    g = geom(c)
    M = g.ntaps * g.Cin
    w4 = wgrad4_kind(c, g)
    if w4:
        splits = wgrad4_slices(c, w4).slabs
        return Plan(10 + w4, 'w4', w4, 0, 0, 0, 0, splits, _zl(splits, M * c.Cout), False)
    variant, bn = (0, 128) if c.Cout > 64 else ((1, 64) if c.Cout > 32 else (2, 32))
    mt, nt = cdiv(M, 128), cdiv(c.Cout, bn)
    steps = cdiv(g.P, BKP)
    kind, kid = 'flat', variant + ((50 if c.flags & 1 else 20) if variant <= 1 else 0)
    cb = 32 if variant == 0 else 64
    steps16 = c.N * g.GH * cdiv(g.GW, BKP)
    if variant <= 1 and halo_ok(c, g, variant):
        kind, kid, mt, steps = 'halo', (40 if c.flags & 1 else 30) + variant, g.Cin // cb, steps16
    if k32_ok(c, g):
        mt, nt = g.Cin // 64, c.Cout // 64
        steps = c.N * cdiv(g.GW, KP32) * g.GH
        tiles = mt * nt
        mtf, ntf = g.Cin // cb, cdiv(c.Cout, 128 if variant == 0 else 64)
        wantf = max(1024 // max(mtf * ntf, 1), 1)
        if wantf > steps16 // 16:
            wantf = max(steps16 // 16, 1)
        wantf = min(wantf, 512)
        max_rows = max(min(128, cdiv(steps16, wantf) * BKP // 32), 8)
        lo = cdiv(steps, max_rows)
        hi = max(steps // 8, lo)
        best, beff = lo, 0.0
        sp = lo
        while sp <= hi and sp <= lo + 1024:
            wg = sp * tiles
            eff = wg / (256.0 * cdiv(wg, 256))
            if eff > beff + 1e-9:
                beff, best = eff, sp
            if eff >= 0.97 and wg >= 256:
                break
            sp += 1
        sps = cdiv(steps, best)
        splits = cdiv(steps, sps)
        return Plan(60, 'k32', variant, mt, nt, steps, sps, splits, _zl(splits, M * c.Cout), c.C2 == 0 and c.aff in (None, 0, 1, 2))
    want = max(1024 // (mt * nt), 1)
    want = min(want, max(steps // 16, 1), 512)
    sps = cdiv(steps, want)
    splits = cdiv(steps, sps)
    return Plan(kid, kind, variant, mt, nt, steps, sps, splits, _zl(splits, M * c.Cout), False)


def _zl(splits, tot):
    """ssg_conv2d_wgrad_f32: wgrad_reduce_kernel<32> for many slabs over few elements, else <8>.  The library has no query for
    this choice: only `splits` is pinned (through the workspace size), so which instantiation a case runs rests on this restatement
    of `splits >= 256 && tot <= 32 * 1024`, not on an observation."""
    return 32 if splits >= 256 and tot <= 32 * 1024 else 8


def workspace_bytes(c):
    g = geom(c)
    return make_plan(c).splits * g.ntaps * g.Cin * c.Cout * 4


# ============================================================================ 3. the fp64 reference
def act32(z, act, slope=LRELU_SLOPE, wrong_sign=False):
    """ssg_act on fp32 values (NaN-propagating forms)."""
    z = f32(z)
    if act == ACT_RELU:
        return np.where(z < 0, F32(0), z)
    if act == ACT_LRELU:
        s = F32(slope)
        return np.where(z > 0, z * s, z) if wrong_sign else np.where(z > 0, z, z * s)
    return z


def x_operand(c, x1, x2, scale=None, shift=None, wrong_sign=False):
    """X [N, H, W, Cin] fp32: in1 (through act(fl32(fma(x, scale, shift))) where in_scale is set, exactly bn_apply's expression)
    and in2 concatenated along the channels."""
    x1 = f32(x1)
    if scale is not None:
        with np.errstate(all='ignore'):
            x1 = act32(preact_emul(x1, scale, shift), c.aff, wrong_sign=wrong_sign)
    return x1 if x2 is None else np.concatenate([x1, f32(x2)], axis=-1)


def _tap_view(Xp, c, g, t):
    """Xp: X zero-padded by 2 rows / columns in front and enough behind; the [N, GH, GW, Cin] operand of tap t."""
    oy, ox = 2 + g.dy[t], 2 + g.dx[t]
    return Xp[:, oy:oy + (g.GH - 1) * c.stride + 1:c.stride, ox:ox + (g.GW - 1) * c.stride + 1:c.stride]


def _padded(X, c, g):
    N, H, W, Cin = X.shape
    HP, WP = max(H, (g.GH - 1) * c.stride + 3) + 4, max(W, (g.GW - 1) * c.stride + 3) + 4
    Xp = np.zeros((N, HP, WP, Cin), dtype=X.dtype)
    Xp[:, 2:2 + H, 2:2 + W] = X
    return Xp


def wgrad_ref(c, x1, x2, dout, scale=None, shift=None, elementwise=False):
    """dw[co, c, ky[t], kx[t]] = sum_{n,gy,gx} dout[n,gy,gx,co] X[n, gy in_sy + dy[t], gx in_sx + dx[t], c] for c < Cin_real, taps
    outside the image read 0 (the zero of the activated tensor).  (dw, mag = sum |dout| |X|), fp64 [Cout, Cin_real, k, k].
    The products of fp32 values are exact in fp64 and the P-term sums err by at most P 2^-53 mag.  elementwise: no BLAS (the
    non-finite cases: 0 * inf = NaN is then certainly IEEE's)."""
    g = geom(c)
    X = x_operand(c, x1, x2, scale, shift).astype(F64)
    Xp = _padded(X, c, g)
    d = np.asarray(dout, dtype=F64).reshape(g.P, c.Cout)
    dw = np.zeros((c.Cout, g.cin_real, c.k, c.k), dtype=F64); mag = np.zeros_like(dw)
    with np.errstate(all='ignore'):
        for t in range(g.ntaps):
            xt = np.ascontiguousarray(_tap_view(Xp, c, g, t)).reshape(g.P, g.Cin)[:, :g.cin_real]
            if elementwise:
                r = np.zeros((c.Cout, g.cin_real)); m = np.zeros_like(r)
                for p0 in range(0, g.P, 256):
                    pr = d[p0:p0 + 256, :, None] * xt[p0:p0 + 256, None, :]
                    r += pr.sum(axis=0); m += np.abs(pr).sum(axis=0)
            else:
                r = d.T @ xt; m = np.abs(d).T @ np.abs(xt)
            dw[:, :, g.ky[t], g.kx[t]] = r; mag[:, :, g.ky[t], g.kx[t]] = m
    return dw, mag


def linear_ref(x, dy):
    """dw[o][k] = sum_n dy[n][o] x[n][k]; (dw, mag)."""
    x = np.asarray(x, dtype=F64); dy = np.asarray(dy, dtype=F64)
    return dy.T @ x, np.abs(dy).T @ np.abs(x)


# ============================================================================ 4. gates
# (b) one product on a split route.  mfma_split.h: x = x1 + x2 + x3 exactly, x1 = bf16(x), x2 = bf16(x - x1), x3 = x - x1 - x2 (8
# significand bits each, round to nearest: |x2| <= 2^-8 |x|, |x3| <= 2^-16 |x|, |x1| <= (1 + 2^-8) |x|); the same for d.  Of the nine
# products the kernels form six, small ones first: d3 x1, d2 x2, d1 x3, d2 x1, d1 x2, d1 x1 (each exact in fp32: 8 x 8 bits).
#   omitted: |d2 x3| + |d3 x2| + |d3 x3| <= (2^-24 + 2^-24 + 2^-32) |x d| = (2 + 2^-8) u32 |x d|;
#   summed:  the first product meets an exact zero; each of the other five additions rounds a partial sum that is at most
#            (1 + 2^-8)^2 |x d| -- at most 5 (1 + 2^-6) u32 |x d| in all, whichever way the matrix unit rounds to within one ulp / 2;
#   7.1 u32 |x d|, and one more u32 |x d| for the second-order terms and the slab sums that meet only zeros: c = 8.
# With d a power of two d2 = d3 = 0 and the sum is (d1 x3 + d1 x2) + d1 x1: x3 + x2 = x - x1 is an fp32 number, so both additions
# are exact; the same with x a power of two.  On the fp32-MFMA routes a single product rounds once: u32 |x d|.
C_SPLIT = 8.0


def product_gate(ref, split):
    return (C_SPLIT if split else 1.0) * U32 * np.abs(np.asarray(ref, dtype=F64))


# (c) hard gate: P = N GH GW products are summed in some order fixed by the route (steps, slabs, the reduce's lanes): each of the
# P - 1 additions rounds a partial sum bounded by mag, P u32 mag for any order; the products are exact inside the matrix units
# and round once on the VALU route (id 17, sum u32 |x d| <= u32 mag); on split routes every product carries C_SPLIT u32 |x d|.
# One more u32 mag covers the second order ((1 + u)^P - 1 - P u, P <= 2^17) and the reference's own P 2^-53 mag; u32 |ref| is the
# final store.  Adding an exact zero (padding, idle slots, empty slabs) costs nothing.
def hard_gate(ref, mag, P, split):
    return (P + 1 + (C_SPLIT if split else 1.0)) * U32 * np.asarray(mag, dtype=F64) + U32 * np.abs(np.asarray(ref, dtype=F64))


RMS_MARGIN = 2.0       # a kernel's RMS error against fp64 over the whole tensor may be at most this many times emul()'s


def rms(err):
    err = np.asarray(err, dtype=F64)
    return float(np.sqrt(np.mean(err * err))) if err.size else 0.0


def classes(a):
    """0 finite, 1 +inf, 2 -inf, 3 NaN."""
    a = np.asarray(a)
    return np.where(np.isnan(a), 3, np.where(np.isposinf(a), 1, np.where(np.isneginf(a), 2, 0)))


def equal_values(got, ref):
    """got (fp32) equals the fp64 reference exactly, element by element (a zero of either sign equals zero)."""
    got = np.asarray(got); ref = np.asarray(ref, dtype=F64)
    return got.shape == ref.shape and bool(np.all(got.astype(F64) == ref))


def first_mismatch(got, ref):
    got = np.asarray(got).astype(F64); ref = np.asarray(ref, dtype=F64)
    bad = np.argwhere(~(got == ref))
    if not len(bad):
        return None
    i = tuple(int(v) for v in bad[0])
    return '%d of %d elements differ, first at (co, c, ky, kx) = %s: got %r, reference %r' % (len(bad), got.size, i, got[i], ref[i])


# ============================================================================ 5. data
def _seed(c, cls):
    return (sum(ord(ch) * (i + 1) for i, ch in enumerate(c.name)) * 7 + cls * 1009) % (2 ** 31)


def _affine(c, rng, integer):
    if c.aff is None:
        return None, None
    if integer:      # scale in {1, 2, -1}, integer shift > 0: a transformed padding pixel would be act(shift) != 0
        return f32(rng.choice([1.0, 2.0, -1.0], c.C1)), f32(rng.randint(1, 4, c.C1))
    return f32(rng.uniform(0.5, 1.5, c.C1) * rng.choice([1.0, -1.0], c.C1)), f32(rng.uniform(0.1, 0.6, c.C1))


def int_data(c):
    """Class (a): x, dout integers in [-irange, irange], scale in {1, 2, -1}, integer shift, slope 1/4: every product and every
    partial sum is a multiple of 1/4 below 2^24 in magnitude (asserted on the magnitude sum by the case table's check) and a single
    bf16 term (|X| <= 2 * 8 + 3 = 19, |4 X| <= 76 < 256)."""
    g = geom(c)
    rng = np.random.RandomState(_seed(c, 1))
    r = c.irange
    x1 = f32(rng.randint(-r, r + 1, (c.N, c.H, c.W, c.C1)))
    x2 = f32(rng.randint(-r, r + 1, (c.N, c.H, c.W, c.C2))) if c.C2 else None
    d = f32(rng.randint(-r, r + 1, (c.N, g.GH, g.GW, c.Cout)))
    sc, sh = _affine(c, rng, True)
    return x1, x2, d, sc, sh


def _full(rng, shape, mean):
    """fp32 values with all 24 significand bits in use: the last bit is set, so the third bf16 term is non-zero."""
    a = f32(mean + rng.standard_normal(shape))
    return (a.view(np.uint32) | np.uint32(1)).view(np.float32)


def rand_data(c):
    """Class (c): full-mantissa operands with non-zero means."""
    g = geom(c)
    rng = np.random.RandomState(_seed(c, 3))
    x1 = _full(rng, (c.N, c.H, c.W, c.C1), 0.3)
    x2 = _full(rng, (c.N, c.H, c.W, c.C2), -0.2) if c.C2 else None
    d = _full(rng, (c.N, g.GH, g.GW, c.Cout), 0.1)
    sc, sh = _affine(c, rng, False)
    return x1, x2, d, sc, sh


def _pow2(rng, shape):
    return f32(np.ldexp(rng.choice([1.0, -1.0], shape), rng.randint(-3, 4, shape)))


def onehot_pixel(c):
    """(n, gy, gx) of the one non-zero dout pixel: the last image, a middle row, and the last column but one (all three columns of
    the window inside the image) -- or the last column where GW % 16 == 1, so that the product lies in the one-column ragged strip
    of the 16- and 32-pixel strip routes (its right-hand taps then read the padding: exact zeros)."""
    g = geom(c)
    return c.N - 1, g.GH // 2, g.GW - 1 if g.GW % 16 == 1 else max(g.GW - 2, 0)


def onehot_data(c, variant):
    """Class (b): dout is non-zero at one pixel of the tensor, so every dw element is a single product (or zero).
    variant 'dpow2': dout powers of two -> dw must be exactly X 2^k; 'xpow2': X powers of two -> exactly dout 2^k; 'full': both full.
    Where the case has a fused input transform it stays on (wgrad_k32_kernel<true>): the scale is a signed power of two, the shift a
    full-mantissa value, or 0 for 'xpow2' so that X = act(x scale) is a power of two or zero."""
    g = geom(c)
    rng = np.random.RandomState(_seed(c, 2))
    mk = lambda shape, p2, mean: _pow2(rng, shape) if p2 else _full(rng, shape, mean)
    x1 = mk((c.N, c.H, c.W, c.C1), variant == 'xpow2', 0.3)
    x2 = mk((c.N, c.H, c.W, c.C2), variant == 'xpow2', -0.2) if c.C2 else None
    d = np.zeros((c.N, g.GH, g.GW, c.Cout), dtype=F32)
    n, gy, gx = onehot_pixel(c)
    d[n, gy, gx] = mk((c.Cout,), variant == 'dpow2', 0.1)
    if c.aff is None:
        return x1, x2, d, None, None
    return x1, x2, d, _pow2(rng, c.C1), np.zeros(c.C1, dtype=F32) if variant == 'xpow2' else _full(rng, c.C1, 0.3)


def nonfinite_data(c, where):
    """rand_data with +inf, NaN and 3.4e38 planted in x (where = 'x': three channels of in1, three pixels) or in dout."""
    g = geom(c)
    x1, x2, d, sc, sh = rand_data(c)
    x1 = x1.copy(); d = d.copy()
    vals = (np.inf, np.nan, 3.4e38)
    if where == 'x':
        for i, v in enumerate(vals):
            x1[c.N - 1, (c.H // 2 + i) % c.H, (c.W - 2 + i) % c.W, (5 + 17 * i) % c.C1] = v
    else:
        for i, v in enumerate(vals):
            d[c.N - 1, (g.GH // 2 + i) % g.GH, (g.GW - 2 + i) % g.GW, (3 + 13 * i) % c.Cout] = v
    return x1, x2, d, sc, sh


# ============================================================================ 6. the case table
def _c(name, N, H, W, C1, C2, Cout, k=3, stride=1, flags=1, k32=1, cin_real=None, ld1=None, ld2=None, ldd=None, aff=None,
       irange=8, stat=False):
    return WgCase(name, N, H, W, C1, C2, Cout, k, stride, flags, k32, cin_real, ld1, ld2, ldd, aff, irange, stat)


def _cases():
    cs = []
    # ---- k32 (id 60): one strip (W 17, 32), a one-column ragged strip (33, 65); H such that steps_per_split does not divide H: a
    # slab starts in the middle of a strip and the rolling window restarts there; a ragged last slab; concat; 128 channels
    cs += [_c('k32_w33_h12', 2, 12, 33, 64, 0, 64, stat=True),
           _c('k32_w17', 1, 19, 17, 64, 0, 64), _c('k32_w32', 2, 9, 32, 64, 0, 64), _c('k32_w65', 1, 11, 65, 64, 0, 64),
           _c('k32_cat', 2, 12, 33, 64, 64, 64), _c('k32_cat_ld', 1, 13, 33, 64, 64, 64, ld1=80, ld2=72, ldd=68, cin_real=125, stat=True),
           _c('k32_c128', 1, 10, 33, 128, 0, 128, stat=True), _c('k32_ragged_slab', 1, 21, 40, 64, 0, 64),
           _c('k32_aff_none', 2, 12, 33, 64, 0, 64, aff=ACT_NONE), _c('k32_aff_relu', 2, 12, 33, 64, 0, 64, aff=ACT_RELU, stat=True),
           _c('k32_aff_lrelu', 1, 13, 33, 64, 0, 64, aff=ACT_LRELU, ld1=72)]
    # ---- halo (30 / 31) and halo_x3 (40 / 41: k32 switched off, or a shape k32 declines: W < 17, Cout % 64 != 0)
    for fl, tag in ((0, 'halo'), (1, 'halox3')):
        cs += [_c('%s_32x128_w17' % tag, 2, 9, 17, 32, 0, 128, flags=fl, k32=0, stat=True),
               _c('%s_64x48_w33' % tag, 2, 9, 33, 64, 0, 48, flags=fl, stat=True),
               _c('%s_w1_h9' % tag, 3, 9, 1, 32, 0, 128, flags=fl), _c('%s_w15_h2' % tag, 2, 2, 15, 64, 0, 48, flags=fl),
               _c('%s_w16_h1' % tag, 2, 1, 16, 64, 0, 64, flags=fl), _c('%s_w33_h1' % tag, 1, 1, 33, 32, 0, 72, flags=fl),
               _c('%s_cat_32' % tag, 2, 9, 17, 32, 64, 96, flags=fl, ld1=40, ld2=64, ldd=100, cin_real=95, stat=bool(fl)),
               _c('%s_cat_64' % tag, 2, 9, 15, 64, 128, 40, flags=fl, ld2=132, cin_real=190, stat=bool(fl)),
               _c('%s_slabs_0' % tag, 2, 23, 33, 32, 0, 128, flags=fl, k32=0), _c('%s_slabs_1' % tag, 2, 23, 33, 64, 0, 64, flags=fl, k32=0)]
    # ---- dma (20 / 21) and dma_x3 (50 / 51): 1x1, stride 2 on odd and even sizes, C % 32 != 0 at stride 1, M % 128 != 0,
    # Cout 33 / 64 / 65 / 80, concat, pixel counts that are no multiple of 16 and below 16
    for fl, tag in ((0, 'dma'), (1, 'dmax3')):
        cs += [_c('%s_1x1_c80' % tag, 2, 7, 9, 24, 0, 80, k=1, flags=fl, stat=True), _c('%s_1x1_c33' % tag, 1, 3, 5, 40, 0, 33, k=1, flags=fl),
               _c('%s_s2_15x17' % tag, 2, 15, 17, 16, 0, 64, stride=2, flags=fl, stat=True), _c('%s_s2_16x16' % tag, 2, 16, 16, 32, 0, 65, stride=2, flags=fl),
               _c('%s_c48' % tag, 2, 9, 11, 48, 0, 80, flags=fl), _c('%s_c96' % tag, 1, 9, 11, 96, 0, 64, flags=fl),
               _c('%s_cat' % tag, 2, 9, 11, 16, 24, 33, flags=fl, ld1=20, ld2=28, ldd=40, cin_real=39, stat=bool(fl)),
               _c('%s_cat_s2' % tag, 2, 9, 10, 24, 16, 72, stride=2, flags=fl, ld2=32, cin_real=38, stat=bool(fl)),
               _c('%s_slabs_0' % tag, 3, 37, 37, 16, 0, 72, k=1, flags=fl), _c('%s_slabs_1' % tag, 3, 37, 37, 16, 0, 40, k=1, flags=fl)]
    # ---- wgrad_kernel<128,32> (id 2): Cout 9 / 24 / 32, Cin 16 / 24, 3x3 at stride 1 and 2, 1x1, an image smaller than one K-step
    cs += [_c('reg_c9', 2, 9, 11, 16, 0, 9, flags=0, stat=True), _c('reg_c24_s2', 2, 9, 11, 24, 0, 24, stride=2), _c('reg_c32_1x1', 2, 7, 9, 16, 0, 32, k=1),
           _c('reg_tiny', 1, 3, 3, 24, 0, 9), _c('reg_cat_ld', 2, 9, 11, 8, 16, 24, ld1=12, ld2=24, ldd=28, cin_real=22),
           _c('reg_cat_s2', 2, 9, 11, 8, 8, 32, stride=2, ld1=16, cin_real=15), _c('reg_slabs', 3, 37, 37, 16, 0, 24, k=1, cin_real=13)]
    # ---- wgrad4: id 15 (Cout <= 4, C1 >= 16: more than one 64-channel group at 128), widths around the 32-pixel segment
    cs += [_c('w4out_c1_16', 2, 5, 31, 16, 0, 1, stat=True), _c('w4out_c3_64', 2, 5, 32, 64, 0, 3), _c('w4out_c4_128', 2, 5, 33, 128, 0, 4, ldd=8, ld1=132, cin_real=126),
           _c('w4out_1x1', 2, 5, 33, 64, 0, 3, k=1), _c('w4out_slabs', 2, 19, 70, 16, 0, 2, cin_real=15)]
    # id 16 (C1 = 4 of which 3 are real), Cout 9 / 64 / 96, 3x3 and 1x1
    cs += [_c('w4in_c9', 2, 5, 31, 4, 0, 9, cin_real=3, stat=True), _c('w4in_c64', 2, 5, 33, 4, 0, 64, cin_real=3), _c('w4in_c96_1x1', 2, 5, 32, 4, 0, 96, k=1, cin_real=3),
           _c('w4in_ld', 2, 5, 33, 4, 0, 68, cin_real=3, ld1=8, ldd=72), _c('w4in_slabs', 2, 19, 70, 4, 0, 40, cin_real=3),
           _c('w4in_reduce32', 2, 128, 128, 4, 0, 64, cin_real=3, irange=4)]
    # id 17 (C1 = 4, Cout <= 8, 3x3): one workgroup with idle slots, and more than one slab with a ragged last one
    cs += [_c('tiny_c1', 1, 5, 7, 4, 0, 1, cin_real=3), _c('tiny_c5', 2, 9, 31, 4, 0, 5, cin_real=3, stat=True), _c('tiny_c8_ld', 1, 70, 67, 4, 0, 8, cin_real=3, ld1=8, ldd=12)]
    # id 18: the smallest tensor with 65536 pixels, integers in [-4, 4]
    cs += [_c('w32cin_c32', 1, 256, 256, 4, 0, 32, cin_real=3, irange=4, stat=True), _c('w32cin_c96_ld', 1, 256, 256, 4, 0, 96, cin_real=3, irange=4, ld1=8, ldd=100),
           # ... and odd widths that are no multiple of the 32-pixel segment (a half-empty last pixel pair) with a slice count that is no
           # multiple of the workgroup's 4 waves (idle waves behind the last unit)
           _c('w32cin_w33', 1, 1987, 33, 4, 0, 32, cin_real=3, irange=4), _c('w32cin_w199_ld', 1, 331, 199, 4, 0, 96, cin_real=3, irange=4, ld1=8, ldd=100)]
    # ---- the linear layer's weight gradient as a 1x1 conv on a 1 x n image (ops.py: _Linear.backward)
    cs += [_c('linear_5_288_1024', 1, 1, 5, 288, 0, 1024, k=1), _c('linear_5_288_1024_fp32', 1, 1, 5, 288, 0, 1024, k=1, flags=0),
           _c('linear_3_1024_1', 1, 1, 3, 1024, 0, 1, k=1)]
    return cs


CASES = _cases()
LINEAR_CASES = [(5, 288, 1024), (3, 1024, 1)]            # ssg_linear_wgrad_f32 on the (n, k, o) of the linear_* conv cases
NONFINITE_CASES = ['k32_w17', 'halox3_w15_h2', 'dmax3_1x1_c33']     # the smallest shape of each split route


def case(name):
    return next(c for c in CASES if c.name == name)


def chains(c, drop_last_strip=False, ragged_too_far=False):
    """The route's partition of the pixels: index arrays [slabs, chains per slab, L] of (n, gy, gx), `live` (the slot holds a pixel)
    and `head` (the slot belongs to the first K-step of a slab that starts below the top row of its strip: the rolling window of
    wgrad_k32 is reloaded there).  One chain is one accumulator's summation order; a slab adds its chains in order.
    drop_last_strip / ragged_too_far: planted defects of the strip routes."""
    g = geom(c); p = make_plan(c)
    head = None
    if p.kind == 'w4' and p.variant == 7:
        i = np.arange(TINY_PIX // 32)
        flat = np.arange(p.splits)[:, None, None] * TINY_PIX + np.arange(32)[None, :, None] + 32 * i[None, None, :]
        live = flat < g.P
    elif p.kind == 'w4':
        s = wgrad4_slices(c, p.variant)
        units = c.N * c.H * s.spr
        z = np.arange(p.splits * 4).reshape(p.splits, 4, 1, 1)
        u = z * s.upz + np.arange(s.upz)[None, None, :, None]
        j = np.arange(SEG)[None, None, None, :]
        gx = (u % s.spr) * SEG + j
        live = (u < np.minimum((z + 1) * s.upz, units)) & (gx < c.W)
        flat = ((u // s.spr) * c.W + gx).reshape(p.splits, 4, -1)
        live = live.reshape(p.splits, 4, -1)
    elif p.kind == 'flat':
        flat = (np.arange(p.splits)[:, None] * p.sps * BKP + np.arange(p.sps * BKP)[None, :])[:, None, :]
        live = flat < np.minimum((np.arange(p.splits)[:, None, None] + 1) * p.sps * BKP, g.P)
    else:
        KPX = STRIP_IDS[p.kid]
        XB = cdiv(g.GW, KPX)
        S = np.arange(p.splits)[:, None] * p.sps + np.arange(p.sps)[None, :]
        live_s = S < p.steps
        gy = S % g.GH; col = S // g.GH
        xb = col % XB; n = col // XB
        j = np.arange(KPX + 1)
        gx = xb[..., None] * KPX + j
        last_ragged = (xb == XB - 1) & (g.GW % KPX != 0)
        lim = np.where(last_ragged & ragged_too_far, g.GW + 1, g.GW)
        live = live_s[..., None] & (j < KPX) & (gx < g.GW)
        if ragged_too_far:
            live = live_s[..., None] & (gx < lim[..., None]) & (j <= KPX)
        if drop_last_strip and XB > 1:
            live &= (xb != XB - 1)[..., None]
        flat = (n[..., None] * g.GH + gy[..., None]) * g.GW + gx            # gx == GW: the next row's first pixel, as the memory lies
        head = np.zeros(S.shape, dtype=bool)
        head[:, 0] = gy[:, 0] > 0
        head = np.broadcast_to(head[..., None], flat.shape).reshape(p.splits, 1, -1)
        flat = flat.reshape(p.splits, 1, -1); live = live.reshape(p.splits, 1, -1)
        n_ = np.broadcast_to(n[..., None], gx.shape).reshape(p.splits, 1, -1)
        gy_ = np.broadcast_to(gy[..., None], gx.shape).reshape(p.splits, 1, -1)
        return n_, gy_, gx.reshape(p.splits, 1, -1), flat, live, head
    flat = np.where(live, flat, 0)
    n = flat // (g.GH * g.GW); rem = flat % (g.GH * g.GW)
    return n, rem // g.GW, rem % g.GW, flat, live, np.zeros(flat.shape, dtype=bool)


def slab_facts(c):
    """Facts of the case's slab partition that check_coverage asks for."""
    g = geom(c); p = make_plan(c)
    facts = set()
    if p.splits > 1:
        facts.add('slabs')
    if p.kind in ('flat', 'halo', 'k32'):
        if p.splits > 1 and p.steps % p.sps:
            facts.add('ragged_slab')
        if p.kind != 'flat' and any((z * p.sps) % g.GH for z in range(1, p.splits)):
            facts.add('mid_strip')
        if p.kind != 'flat' and g.GW % STRIP_IDS[p.kid]:
            facts.add('ragged_strip')
        if p.kind == 'flat' and g.P % BKP:
            facts.add('ragged_step')
    elif p.variant == 7:
        if g.P % TINY_PIX:
            facts.add('ragged_slab')
    else:
        s = wgrad4_slices(c, p.variant)
        if s.waves % 4 or (c.N * c.H * s.spr) % s.upz:
            facts.add('ragged_slab')
        if c.W % SEG:
            facts.add('ragged_strip')
    if c.C2:
        facts.add('concat')
    if g.ld1 > c.C1 or g.ldd > pad4(c.Cout) or (c.C2 and g.ld2 > c.C2):
        facts.add('ld')
    if c.C2 and g.ld2 != g.ld1:
        facts.add('ld2!=ld1')
    if g.cin_real < g.Cin:
        facts.add('pad_channels')
    if c.stride == 2:
        facts.add('stride2')
    if c.k == 1:
        facts.add('1x1')
    return facts


# what each route accepts (beyond 'slabs', 'ld' and 'pad_channels', which every route does)
ROUTE_FEATURES = {2: {'concat', 'stride2', '1x1', 'ragged_slab', 'ragged_step'},
                  20: {'concat', 'stride2', '1x1', 'ragged_slab', 'ragged_step'}, 21: {'concat', 'stride2', '1x1', 'ragged_slab', 'ragged_step'},
                  50: {'concat', 'stride2', '1x1', 'ragged_slab', 'ragged_step'}, 51: {'concat', 'stride2', '1x1', 'ragged_slab', 'ragged_step'},
                  30: {'concat', 'ragged_slab', 'mid_strip', 'ragged_strip'}, 31: {'concat', 'ragged_slab', 'mid_strip', 'ragged_strip'},
                  40: {'concat', 'ragged_slab', 'mid_strip', 'ragged_strip'}, 41: {'concat', 'ragged_slab', 'mid_strip', 'ragged_strip'},
                  60: {'concat', 'ragged_slab', 'mid_strip', 'ragged_strip', 'ld2!=ld1'},
                  15: {'1x1', 'ragged_slab', 'ragged_strip'}, 16: {'1x1', 'ragged_slab', 'ragged_strip'}, 17: {'ragged_slab'},
                  18: {'ragged_slab', 'ragged_strip'}}


def check_coverage():
    """The table reaches every reachable kernel id x every feature that route accepts, both wgrad_reduce_kernel instantiations (by
    the restated rule of _zl, which no query of the library confirms),
    the fused input transform of wgrad_k32_kernel<true> with each activation, and class (b) and the RMS gate on every id.
    Returns {id: set of facts}."""
    hit, zls, acts, stat = {}, set(), set(), set()
    names = set()
    for c in CASES:
        assert c.name not in names, c.name
        names.add(c.name)
        g = geom(c); p = make_plan(c)
        assert g.GH >= 1 and g.GW >= 1 and c.C1 % 4 == 0 and c.C2 % 4 == 0 and g.ldd >= pad4(c.Cout), c.name
        assert p.kid in REACHABLE_IDS, (c.name, p.kid)
        hit.setdefault(p.kid, set()).update(slab_facts(c))
        zls.add(p.zl)
        if c.aff is not None:
            assert p.aff_ok, c.name
            acts.add(c.aff)
        if c.stat:
            stat.add(p.kid)
    for kid in REACHABLE_IDS:
        assert kid in hit, 'no case reaches kernel id %d' % kid
        need = ROUTE_FEATURES[kid] | {'ld', 'pad_channels', 'slabs'}
        assert need <= hit[kid], 'kernel id %d: no case with %s' % (kid, sorted(need - hit[kid]))
    assert zls == {8, 32}, zls
    assert acts == {ACT_NONE, ACT_RELU, ACT_LRELU}, acts
    assert stat == set(REACHABLE_IDS), sorted(set(REACHABLE_IDS) - stat)
    return hit


def int_class_is_exact(c, mag):
    """Class (a): sum |terms| < 2^24 in units of the smallest term (1, or 1/4 with the leaky slope)."""
    unit = 0.25 if c.aff == ACT_LRELU else 1.0
    return float(np.max(mag)) / unit < 2 ** 24


# ============================================================================ 7. the float32 emulation
def split3(a):
    """mfma_split.h: three bf16 terms of an fp32 array (as fp32), a1 + a2 + a3 == a exactly."""
    a = f32(a)
    a1 = bf16_rne(a); r = a - a1
    a2 = bf16_rne(r)
    return a1, a2, bf16_rne(r - a2)


def reduce_emul(slabs, zl, drop_last_slab=False):
    """wgrad_reduce_kernel<ZL>: lane z adds slabs z, z + ZL, ... in order, then the ZL lane sums are added in lane order, fp32."""
    slabs = f32(slabs)
    if drop_last_slab and slabs.shape[0] > 1:
        slabs = slabs[:-1]
    lanes = np.zeros((zl,) + slabs.shape[1:], dtype=F32)
    for z in range(slabs.shape[0]):
        lanes[z % zl] = lanes[z % zl] + slabs[z]
    v = np.zeros(slabs.shape[1:], dtype=F32)
    for k in range(zl):
        v = v + lanes[k]
    return v


def emul(c, x1, x2, dout, scale=None, shift=None, drop_last_strip=False, ragged_too_far=False, stale_window=False,
         drop_last_slab=False, in2_block_off=False, kykx_transposed=False, pad_written=False, xform_padding=False,
         lrelu_wrong_sign=False, drop_x3=False, drop_x2d2=False, unit_stride_taps=False):
    """The weight gradient in float32 with the route's own partition: every chain of chains(c) adds its pixels' products one by one
    into an fp32 accumulator (fp32 routes: one fused multiply-add per pixel; split routes: the six bf16-term products of
    mfma_split.h, small ones first, each added in fp32), a slab adds its chains in order, reduce_emul adds the slabs, and the
    result is scattered to [Cout][Cin_real][ky][kx].  Returns the flat fp32 gradient followed by 64 NaN guard elements.
    Defects (all off): the last column strip dropped; the ragged strip read one pixel too far; the three-row window not reloaded at
    a slab that starts in the middle of a strip (its row above reads as zeros); the last slab dropped; in2's channels read one
    channel block further; ky / kx transposed; pad channels written; the input transform applied to padding pixels; the leaky
    slope on the wrong sign; the third bf16 term of x dropped; the x2 d2 product dropped; stride-2 taps read at unit stride."""
    g = geom(c); p = make_plan(c)
    split = p.kid in SPLIT_IDS
    if in2_block_off and x2 is not None:
        blk = 64 if p.kind == 'k32' else (32 if p.kind == 'halo' and p.variant == 0 else (64 if p.kind == 'halo' else 4))
        fl = f32(x2).reshape(-1)
        x2 = np.concatenate([fl[blk:], np.zeros(blk, dtype=F32)]).reshape(np.shape(x2))
    X = x_operand(c, x1, x2, scale, shift, wrong_sign=lrelu_wrong_sign)
    padval = np.zeros(g.Cin, dtype=F32)
    if xform_padding and scale is not None:
        padval[:c.C1] = act32(f32(shift), c.aff, wrong_sign=lrelu_wrong_sign)
    n, gy, gx, flat, live, head = chains(c, drop_last_strip, ragged_too_far)
    dflat = np.concatenate([f32(dout).reshape(g.P, c.Cout), np.zeros((1, c.Cout), dtype=F32)])
    s = 1 if unit_stride_taps else c.stride
    nsl, nch, L = flat.shape
    acc = np.zeros((nsl, nch, g.ntaps, g.Cin, c.Cout), dtype=F32)
    terms = ((2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0))        # (d term, x term): d3 x1, d2 x2, d1 x3, d2 x1, d1 x2, d1 x1
    with np.errstate(all='ignore'):
        for l in range(L):
            lv = live[:, :, l]
            if not lv.any():
                continue
            d = dflat[np.where(lv & (flat[:, :, l] < g.P), flat[:, :, l], g.P)]                      # [nsl, nch, Cout]
            ds = split3(d) if split else None
            for t in range(g.ntaps):
                iy = gy[:, :, l] * s + g.dy[t]; ix = gx[:, :, l] * s + g.dx[t]
                inside = lv & (iy >= 0) & (iy < c.H) & (ix >= 0) & (ix < c.W)
                xt = np.where(inside[..., None], X[np.clip(n[:, :, l], 0, c.N - 1), np.clip(iy, 0, c.H - 1), np.clip(ix, 0, c.W - 1)], padval)
                xt = np.where(lv[..., None], xt, F32(0))
                if stale_window and g.dy[t] == -1:
                    xt = np.where(head[:, :, l][..., None], F32(0), xt)
                if split:
                    xs = list(split3(xt))
                    if drop_x3:
                        xs[2] = np.zeros_like(xs[2])
                    for (qd, qx) in terms:
                        if drop_x2d2 and (qd, qx) == (1, 1):
                            continue
                        acc[:, :, t] = acc[:, :, t] + xs[qx][..., :, None] * ds[qd][..., None, :]
                else:
                    acc[:, :, t] = (acc[:, :, t].astype(F64) + xt.astype(F64)[..., :, None] * d.astype(F64)[..., None, :]).astype(F32)
        slabs = np.zeros((nsl, g.ntaps, g.Cin, c.Cout), dtype=F32)
        for k in range(nch):
            slabs = slabs + acc[:, k]
        v = reduce_emul(slabs, p.zl, drop_last_slab)                 # [ntaps, Cin, Cout]
    out = np.full(c.Cout * g.cin_real * c.k * c.k + 64, np.nan, dtype=F32)
    KH = KW = c.k
    for t in range(g.ntaps):
        ky, kx = (g.kx[t], g.ky[t]) if kykx_transposed else (g.ky[t], g.kx[t])
        for ci in range(g.Cin if pad_written else g.cin_real):
            idx = ((np.arange(c.Cout) * g.cin_real + ci) * KH + ky) * KW + kx
            if ci >= g.cin_real:                                     # a pad channel's element lands on a real one further on, or past the end
                keep = idx < out.size
                out[idx[keep]] = v[t, ci][keep]
            else:
                out[idx] = v[t, ci]
    return out


def emul_dw(c, out):
    """(dw [Cout, Cin_real, k, k], guard intact) of emul()'s flat result."""
    g = geom(c)
    n = c.Cout * g.cin_real * c.k * c.k
    return out[:n].reshape(c.Cout, g.cin_real, c.k, c.k), bool(np.isnan(out[n:]).all())


# ============================================================================ 8. the descriptor of a case
def fill_desc(d, c, in1, in2, dout, dw, ws=None, ws_bytes=0, scale=None, shift=None):
    """Fill the ssg_wgrad_desc `d` (a fresh _lib.WgradDesc) for case c with the given addresses, as ops._conv_wgrad_impl fills it."""
    g = geom(c)
    d.in1 = in1; d.C1 = c.C1; d.ld1 = g.ld1
    d.in2 = in2 if c.C2 else None; d.C2 = c.C2; d.ld2 = g.ld2 if c.C2 else 0
    d.N, d.H, d.W = c.N, c.H, c.W
    d.dout = dout; d.Cout = c.Cout; d.ldd = g.ldd; d.GH, d.GW = g.GH, g.GW
    d.in_sy = d.in_sx = c.stride
    d.ntaps = g.ntaps
    for t in range(g.ntaps):
        d.dy[t], d.dx[t], d.ky[t], d.kx[t] = g.dy[t], g.dx[t], g.ky[t], g.kx[t]
    d.KH = d.KW = c.k; d.Cin_real = g.cin_real
    d.dw_oihw = dw
    d.ws = ws; d.ws_bytes = ws_bytes
    d.flags = c.flags
    d.in_scale = scale if c.aff is not None else None; d.in_shift = shift if c.aff is not None else None
    d.in_act = c.aff or 0; d.in_slope = LRELU_SLOPE if c.aff == ACT_LRELU else 0.0
    return d
