"""Reference for the opt-in bf16x1 STRIDE-2 weight gradient (csrc/conv_wgrad_s2_k32_x1.hip, ssg_conv2d_wgrad_bf16x1_s2_f32).
Plain helper module (not a conftest), numpy only, built on wgrad_ref (whose fp64 reference, data classes and descriptor already
take stride = 2) and on wgrad_x1_ref's gates: nothing here calls an op under test.

The arithmetic is wgrad_k32_x1_kernel's: x and dout rounded ONCE to bf16 (round to nearest even), products exact in fp32, fp32 sums.
So the two gates of wgrad_x1_ref hold unchanged with P = N GH GW OUTPUT pixels: (P + 2) u32 mag + u32 |ref| against fp64 on the
rounded operands, and that plus (2^-8 + 2^-18) sum |x| |dout| against fp64 on the operands as given.

What is new is the addressing.  A K-step is 32 output pixels ox0 .. ox0 + 31 of output row oy; steps are numbered
S = (image * XB + strip) * GH + oy; slab z sums steps [z * sps, (z + 1) * sps).  x row r = 2 oy + ky - 1 is staged as two planes,
E[j] = x[r, 2 (ox0 + j)] (j = 0..31) and O[j] = x[r, 2 (ox0 + j) - 1] (j = 0..32), zero outside the image; tap kx = 0, 1, 2 of output
pixel j reads O[j], E[j], O[j + 1].  emul() is written in exactly those terms, so that its keyword switches -- the planted defects
of tests/test_wgrad_s2_x1_ref.py, all off -- are the mistakes this addressing can make."""
import numpy as np

import wgrad_ref as wr
import wgrad_x1_ref as xr
from wgrad_ref import F32, F64, bf16_rne, f32

KERNEL_IDS = {128: 81, 64: 82}             # by Cout % 128: wgrad_s2_k32_x1_kernel<4> / <2>
FP32_IDS = (50, 51)                        # what ssg_conv2d_wgrad_f32 runs on these shapes (wgrad_dma_x3)
KP = xr.KP
BOUND = xr.BOUND


def _c(name, N, H, W, Cin, Cout, **kw):
    return wr._c(name, N, H, W, Cin, 0, Cout, stride=2, irange=3, **kw)


# (N, H, W, Cin, Cout): the smallest shapes at which this kernel can go wrong
CASES = [
    _c('s2_w33_h5', 1, 5, 33, 64, 64),               # GW = 17 minimum; odd H and W: right and bottom padding are read; GH = 3
    _c('s2_w34_h4_c128', 1, 4, 34, 64, 128),         # even sizes, last tap column W - 1 inside, NJ = 4
    _c('s2_w79_cin128', 1, 6, 79, 128, 64),          # GW = 40: a second strip 8 wide; two input-channel tiles
    _c('s2_w64_h2', 1, 2, 64, 64, 64),               # GW = 32: exactly one full strip; GH = 1
    _c('s2_slabs', 3, 37, 66, 64, 128),              # GW = 33: a one-column strip; several slabs, ragged last
    _c('s2_ld', 1, 4, 34, 64, 64, ld1=72, ldd=136),  # the second case's geometry as channel slices of NaN-filled rows
]
SLABS = 's2_slabs'
NONFINITE_CASE = 's2_w79_cin128'


def case(name):
    return next(c for c in CASES if c.name == name)


def kernel_id(c):
    return KERNEL_IDS[128 if c.Cout % 128 == 0 else 64]


def plan(c):
    """ssg_wgrad_bf16_plan of csrc/conv_k32_bf16_host.h at stride 2 (8 .. 128 K-steps per slab, fewest idle CUs in the last wave) on
    steps = N * ceil(GW / 32) * GH of the OUTPUT grid -- wgrad_x1_ref.plan reads GH / GW from wgrad_ref.geom, which are the output's at
    stride 2.  (nj, mt, nt, steps, steps_per_split, splits)."""
    return xr.plan(c)


def workspace_bytes(c):
    return plan(c)[5] * 9 * c.C1 * c.Cout * 4


def ok(c):
    """ssg_conv2d_wgrad_bf16x1_s2_ok restated for a WgCase."""
    g = wr.geom(c)
    return (c.k == 3 and c.stride == 2 and c.aff is None and c.C1 > 0 and c.C1 % 64 == 0 and c.C2 == 0 and c.Cout > 0
            and c.Cout % 64 == 0 and g.GH == (c.H + 1) // 2 and g.GW == (c.W + 1) // 2 and g.GW >= 17 and g.cin_real == c.C1
            and g.ld1 % 4 == 0 and g.ld1 >= c.C1 and g.ldd % 4 == 0 and g.ldd >= c.Cout
            and c.N * c.H * c.W * g.ld1 * 4 <= 0xfffffff0 and g.P * g.ldd * 4 <= 0xfffffff0)


def ref_rounded(c, data):
    return xr.ref_rounded(c, data)


def ref_exact(c, data):
    return xr.ref_exact(c, data)


gate_rounded = xr.gate_rounded
gate_exact = xr.gate_exact


def onehot_data(c, where):
    """Class (b): full-mantissa operands, dout non-zero at ONE pixel of the last image.  where = 'interior': a middle row and the
    last column but one of the first strip's interior (every tap inside the image); 'edge': the last row and the last column, whose
    taps reach the bottom / right padding where H / W is odd."""
    g = wr.geom(c)
    rng = np.random.RandomState(wr._seed(c, 2 if where == 'interior' else 4))
    x1 = wr._full(rng, (c.N, c.H, c.W, c.C1), 0.3)
    d = np.zeros((c.N, g.GH, g.GW, c.Cout), dtype=F32)
    oy, ox = (g.GH // 2, max(g.GW - 2, 0)) if where == 'interior' else (g.GH - 1, g.GW - 1)
    d[c.N - 1, oy, ox] = wr._full(rng, (c.Cout,), 0.1)
    return x1, None, d, None, None


def _row_planes(X, n, r, ox0, c, right_pad_nonzero=False, bottom_pad_nonzero=False):
    """(E [32, Cin], O [33, Cin]) of x row r for the strip at ox0, fp64, zeros outside the image.  Defects: the column W / the row
    H read the last column / row instead of zero."""
    Cin = X.shape[-1]
    E = np.zeros((KP, Cin), dtype=F64); O = np.zeros((KP + 1, Cin), dtype=F64)
    if r == c.H and bottom_pad_nonzero:
        r = c.H - 1
    if not 0 <= r < c.H:
        return E, O
    def px(col):
        if col == c.W and right_pad_nonzero:
            col = c.W - 1
        return X[n, r, col] if 0 <= col < c.W else 0.0
    for j in range(KP):
        E[j] = px(2 * (ox0 + j))
    for j in range(KP + 1):
        O[j] = px(2 * (ox0 + j) - 1)
    return E, O


def emul(c, data, unit_stride_taps=False, odd_off_by_one=False, swap_planes=False, row_off_by_one=False,
         right_pad_nonzero=False, bottom_pad_nonzero=False, drop_ragged_step=False):
    """The weight gradient in float32 with the kernel's arithmetic and addressing: operands rounded to bf16, a step adds the exact
    products of its (up to) 32 pixels to the slab's fp32 accumulator in K-step order, wgrad_reduce_kernel<8> adds the slabs in order.
    [Cout, Cin, 3, 3] fp32.  Defects (all off): taps read at unit stride (x[oy + ky - 1, ox + kx - 1]); tap kx = 2 reads O[j]; the
    even and odd planes swapped; x row 2 oy + ky; the right pad column / the bottom pad row not zero; the last step of a slab that
    ends ragged (the last slab, shorter than the others) dropped."""
    g = wr.geom(c)
    x1, _, d, _, _ = data
    X = bf16_rne(x1).astype(F64)
    D = bf16_rne(d).astype(F64)
    _, _, _, steps, sps, splits = plan(c)
    XB = wr.cdiv(g.GW, KP)
    slabs = np.zeros((splits, 9, c.C1, c.Cout), dtype=F32)
    for S in range(steps):
        z = S // sps
        if drop_ragged_step and z == splits - 1 and steps % sps and S == steps - 1:
            continue
        col, oy = divmod(S, g.GH)
        n, xb = divmod(col, XB)
        ox0 = xb * KP
        npx = min(KP, g.GW - ox0)
        dr = np.zeros((KP, c.Cout), dtype=F64)
        dr[:npx] = D[n, oy, ox0:ox0 + npx]                               # idle pixels of a ragged strip: zeros
        for ky in range(3):
            if unit_stride_taps:
                r = oy + ky - 1
                row = np.zeros((KP + 2, c.C1), dtype=F64)
                if 0 <= r < c.H:
                    for j in range(KP + 2):
                        col_ = ox0 + j - 1
                        if 0 <= col_ < c.W:
                            row[j] = X[n, r, col_]
                taps = [row[0:KP], row[1:KP + 1], row[2:KP + 2]]
            else:
                r = 2 * oy + ky - (0 if row_off_by_one else 1)
                E, O = _row_planes(X, n, r, ox0, c, right_pad_nonzero, bottom_pad_nonzero)
                if swap_planes:
                    E33 = np.zeros((KP + 1, c.C1), dtype=F64); E33[:KP] = E
                    if 0 <= r < c.H and 2 * (ox0 + KP) < c.W:
                        E33[KP] = X[n, r, 2 * (ox0 + KP)]
                    taps = [E33[0:KP], O[0:KP], E33[1:KP + 1]]
                else:
                    taps = [O[0:KP], E, O[0:KP] if odd_off_by_one else O[1:KP + 1]]
            for kx in range(3):
                t = ky * 3 + kx
                slabs[z, t] = (slabs[z, t].astype(F64) + taps[kx].T @ dr).astype(F32)
    v = wr.reduce_emul(slabs, 8)                                          # [9, Cin, Cout]
    return np.ascontiguousarray(v.reshape(3, 3, c.C1, c.Cout).transpose(3, 2, 0, 1))


def nonfinite_data(c):
    """rand_data clipped to |v| <= 0.9 (no fp32 product of a planted finite value overflows) with 3.4e38 (rounds to bf16
    infinity), 3.39e38 (stays finite), +inf, -inf and NaN planted in x and in dout, each once against a zero partner and once
    against a non-zero one.  Image 0: dout is zero on output rows 0..1, columns 0..7 (x values at input row 1, columns 1, 3, ..:
    every output pixel whose window holds them lies in the island), and x is zero on input rows 2..6, columns 30..50 (dout values
    at output row 2, columns 17..21: their windows lie in it)."""
    g = wr.geom(c)
    assert c.N >= 1 and g.GH >= 3 and g.GW >= 24 and c.H >= 6 and c.W >= 52
    x1, x2, d, sc, sh = wr.rand_data(c)
    x1 = np.clip(x1, -0.9, 0.9).astype(F32); d = np.clip(d, -0.9, 0.9).astype(F32)
    vals = (3.4e38, 3.39e38, np.inf, -np.inf, np.nan)
    d[0, 0:2, 0:8] = 0
    x1[0, 2:c.H, 30:51] = 0
    for i, v in enumerate(vals):
        x1[0, 1, 1 + 2 * i, (3 + 11 * i) % c.C1] = v                     # against zero dout (output rows 0..1, columns 0..5)
        x1[c.N - 1, c.H - 2, 11 + 2 * i, (5 + 13 * i) % c.C1] = v         # against non-zero dout
        d[0, 2, 17 + i, (2 + 7 * i) % c.Cout] = v                         # against zero x (rows 3..5, columns 33..44)
        d[c.N - 1, 0, g.GW - 2 - i, (4 + 9 * i) % c.Cout] = v             # against non-zero x
    return x1, x2, d, sc, sh
