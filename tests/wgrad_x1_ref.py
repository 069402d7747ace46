"""Reference for the opt-in bf16x1 weight gradient (csrc/conv_wgrad_k32_bf16.hip, ssg_conv2d_wgrad_bf16x1_f32).  Plain helper
module (not a conftest), numpy only, built on wgrad_ref: nothing here calls an op under test.

The kernel rounds x and dout ONCE to bf16 (round to nearest even) on the way into LDS and accumulates in fp32.  A product of two
bf16 values has 16 significand bits: it is exact in fp32.  So

* against fp64 on the ROUNDED operands (ref_rounded) the kernel errs by fp32 accumulation alone.  The slab structure as built:
  a K-step is 32 pixels of one image row of a 32-pixel column strip, steps are numbered S = (image * XB + strip) * GH + row, slab
  z sums steps [z * sps, (z + 1) * sps) in one accumulator (at most 128 steps, plan()), wgrad_reduce_kernel adds the slabs.  That
  is one summation tree over the P = N GH GW products of an element plus exact zeros (padding, the idle pixels of a ragged strip):
  P - 1 roundings of partial sums bounded by mag whatever the order, so the slab partition moves no term of the bound -- it is
  wgrad_ref.hard_gate with exact products, (P + 2) u32 mag + u32 |ref| (one u32 mag for second order and the reference's own
  error, one for the products term that hard_gate charges every route);
* against fp64 on the UNROUNDED operands add (2^-8 + 2^-18) sum |x| |dout|: unit roundoff 2^-9 per operand,
  (1 + 2^-9)^2 - 1 (bf16x1_ref.BOUND).

emul() is the float32 emulation with the kernel's slab partition; its keyword switches are the planted defects of
tests/test_wgrad_x1_ref.py (all off)."""
import numpy as np

import wgrad_ref as wr
from bn_ref import bf16_trunc
from wgrad_ref import F32, F64, U32, bf16_rne, f32

KERNEL_ID = 72
KP, MAX_ROWS, MIN_ROWS = 32, 128, 8
BOUND = 2.0 ** -8 + 2.0 ** -18
FLT_MAX = wr.FLT_MAX


def _c(name, N, H, W, C1, C2, Cout, **kw):
    return wr._c(name, N, H, W, C1, C2, Cout, irange=3, **kw)


# N = 1 and 3 (slabs ragged across images); widths 17 (minimum), 33 (a full strip plus one pixel), 40, 64 (two full strips);
# 64+0, 64+64 and 128+0 input channels; both output tiles (64: NJ = 2, 128: NJ = 4); channel slices of wider rows; a ragged last slab.
CASES = [
    _c('x1_w17', 1, 3, 17, 64, 0, 64),
    _c('x1_w33_n3_cat', 3, 5, 33, 64, 64, 128),
    _c('x1_w40_n3_c128', 3, 9, 40, 128, 0, 64),
    _c('x1_w64', 1, 2, 64, 64, 0, 128),
    _c('x1_w40_c128_128', 1, 9, 40, 128, 0, 128),
    _c('x1_cat_ld', 3, 5, 33, 64, 64, 64, ld1=80, ld2=72, ldd=68),
    _c('x1_ragged_slab', 3, 7, 33, 64, 0, 128, ldd=136),
]
RAGGED = 'x1_ragged_slab'          # 42 steps in slabs of 9: five slabs, the last of 6; slabs start in the middle of a strip
NONFINITE_CASE = 'x1_w33_n3_cat'


def case(name):
    return next(c for c in CASES if c.name == name)


def plan(c):
    """ssg_wgrad_bf16_plan of csrc/conv_k32_bf16_host.h restated: (nj, mt, nt, steps, steps_per_split, splits)."""
    g = wr.geom(c)
    nj = 4 if c.Cout % 128 == 0 else 2
    mt, nt = g.Cin // 64, c.Cout // (32 * nj)
    steps = c.N * wr.cdiv(g.GW, KP) * g.GH
    tiles = mt * nt
    lo = wr.cdiv(steps, MAX_ROWS)
    hi = max(lo, steps // MIN_ROWS)
    best, beff = lo, 0.0
    sp = lo
    while sp <= hi and sp <= lo + 1024:
        wg = sp * tiles
        eff = wg / (256.0 * ((wg + 255) // 256))
        if eff > beff + 1e-9:
            beff, best = eff, sp
        if eff >= 0.97 and wg >= 256:
            break
        sp += 1
    sps = wr.cdiv(steps, best)
    return nj, mt, nt, steps, sps, wr.cdiv(steps, sps)


def workspace_bytes(c):
    g = wr.geom(c)
    return plan(c)[5] * 9 * g.Cin * c.Cout * 4


def ok(c):
    """ssg_conv2d_wgrad_bf16x1_ok restated for a WgCase (dense or given strides, no in_scale)."""
    g = wr.geom(c)
    return (c.k == 3 and c.stride == 1 and c.aff is None and c.C1 > 0 and c.C1 % 64 == 0 and c.C2 % 64 == 0 and c.Cout % 64 == 0
            and g.GW >= 17 and g.cin_real == g.Cin)


def rounded(data, rnd=bf16_rne, round_x=True, round_d=True):
    x1, x2, d, sc, sh = data
    rx = rnd if round_x else f32
    rd = rnd if round_d else f32
    return rx(x1), None if x2 is None else rx(x2), rd(d), sc, sh


def ref_rounded(c, data):
    """(dw, mag) in fp64 on the bf16-rounded operands."""
    x1, x2, d, _, _ = rounded(data)
    return wr.wgrad_ref(c, x1, x2, d)


def ref_exact(c, data):
    """(dw, mag) in fp64 on the operands as given."""
    x1, x2, d, _, _ = data
    return wr.wgrad_ref(c, x1, x2, d)


def gate_rounded(c, ref, mag):
    return wr.hard_gate(ref, mag, wr.geom(c).P, False)


def gate_exact(c, ref_r, mag_r, mag):
    return gate_rounded(c, ref_r, mag_r) + BOUND * np.asarray(mag, dtype=F64)


def emul(c, data, unrounded_x=False, truncate=False, drop_tap=None, swap_planes=False, drop_last_slab=False):
    """The weight gradient in float32 with the kernel's partition: a step adds the 32 products of its row (summed exactly: the
    matrix unit's wide adder) to the slab's fp32 accumulator, wgrad_reduce_kernel<8> adds the slabs.  [Cout, Cin, 3, 3] fp32.
    Defects: x left unrounded; truncation instead of round to nearest even; tap `drop_tap` never accumulated; the x fragments read
    from dout's rounded plane (input channel ci sees dout's channel ci mod Cout at the same pixel); the last slab lost."""
    g = wr.geom(c)
    x1, x2, d, _, _ = data
    rnd = bf16_trunc if truncate else bf16_rne
    if swap_planes:
        D = rnd(d)
        X = np.ascontiguousarray(D[..., np.arange(g.Cin) % c.Cout])
    else:
        X = f32(wr.x_operand(c, x1, x2)) if unrounded_x else rnd(wr.x_operand(c, x1, x2))
        D = rnd(d)
    Xp = wr._padded(X.astype(F64), c, g)
    D = D.astype(F64)
    _, _, _, steps, sps, splits = plan(c)
    XB = wr.cdiv(g.GW, KP)
    slabs = np.zeros((splits, 9, g.Cin, c.Cout), dtype=F32)
    for S in range(steps):
        z = S // sps
        col, gy = divmod(S, g.GH)
        n, xb = divmod(col, XB)
        gx0, gx1 = xb * KP, min((xb + 1) * KP, g.GW)
        dr = D[n, gy, gx0:gx1]                                           # [px, Cout]
        for t in range(9):
            if t == drop_tap:
                continue
            xt = Xp[n, 2 + gy + g.dy[t], 2 + g.dx[t] + gx0:2 + g.dx[t] + gx1]   # [px, Cin]
            slabs[z, t] = (slabs[z, t].astype(F64) + xt.T @ dr).astype(F32)
    v = wr.reduce_emul(slabs, 8, drop_last_slab)                          # [9, Cin, Cout]
    return np.ascontiguousarray(v.reshape(3, 3, g.Cin, c.Cout).transpose(3, 2, 0, 1))


def nonfinite_data(c):
    """rand_data with 3.4e38 (rounds to bf16 infinity), 3.39e38 (stays finite), +inf, -inf and NaN planted in x, each at two
    pixels: one whose dout pixel is zero on every channel (and zero on the eight neighbours that share the x value through a tap),
    one in the full-mantissa field.  |dout| < 1 at the planted values' neighbours, so no fp32 product overflows."""
    g = wr.geom(c)
    x1, x2, d, sc, sh = wr.rand_data(c)
    x1 = x1.copy(); d = np.clip(d, -0.9, 0.9).astype(F32)
    vals = (3.4e38, 3.39e38, np.inf, -np.inf, np.nan)
    # zero island: image 0, rows 0..2, columns 0..6 of dout are zero; the values sit inside it at row 1, columns 1..5
    d[0, 0:3, 0:7] = 0
    for i, v in enumerate(vals):
        x1[0, 1, 1 + i, (3 + 11 * i) % c.C1] = v                         # against zero dout
        x1[c.N - 1, g.GH - 2, g.GW - 2 - 2 * i, (5 + 13 * i) % c.C1] = v  # against non-zero dout
    return x1, x2, d, sc, sh
