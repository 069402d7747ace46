"""Plain references for the frozen (running-statistics) batch-norm backward of csrc/bn.hip: ssg_bn_frozen_bwd_f32 (col_reduce_kernel<3>:
the masked gradient, dx = g scale, dres = g and the two column sums in one sweep) and ssg_bn_fold_bwd_f32 (gradients through the fold of a
frozen batch norm into its conv).  Same four kinds of thing as tests/bn_ref.py, which it builds on: numpy and CPU torch only, nothing
here calls an op under test.

Gates (each exact, or a rounding count times a unit roundoff times a magnitude; none fitted):

* sums   -- the kernel shares MODE 1's accumulation expressions: bit-identical to ssg_bn_bwd_reduce_f32 on the same inputs (GPU file), and
            against fp64 bn_ref.sum_gate with bn_ref's counts (k_sum additions; 3 more roundings inside a g xhat term).
* dres   -- the fp32 masked gradient, bit for bit: dy where the output is > 0, else the fp32 product dy * 0 or dy * slope (one rounding,
            which the reference forms the same way).  Swish: bn_ref.swish_grad_gate through |dy|, plus the product's rounding.
* dx     -- fl32(g * scale): ONE fp32 rounding of the fp64 product of the fp32 g and the fp32 scale.  Against the fp64 expression
            dy * slope * scale, LeakyReLU's negative side carries the rounding of dy * slope as well: two there.
* fold   -- dw[o,k] = fl32(dwf[o,k] * s[o]) exactly.  dgamma = fl32((t - mean sum_g) invstd), t = sum_k dwf w: every product is exact in fp64
            (24 + 24 bits), so the error is that of the fp64 additions: ceil(K / 256) per thread + 8 tree levels, far inside the
            2^-50 = 8 u64 relative to sum |dwf w| + |mean sum_g| that the gate grants (a random-walk of at most 35 roundings each well
            below the magnitude sum; the worst case of 35 u64 would need every partial sum to sit at the full magnitude sum with
            every rounding in the same direction); one fp32 rounding of the result.  dbeta = fl32(sum_g): one rounding."""
import numpy as np

import bn_ref as br
from bn_ref import ACT_LRELU, ACT_NONE, ACT_RELU, ACT_SWISH, DENORM, F32, F64, U32, f32, same_bits, worst_ratio

SLOPE = 0.2
ACTS = (ACT_NONE, ACT_RELU, ACT_LRELU, ACT_SWISH)
FOLD_BLOCK = 256
FOLD_CASES = [(4, 27), (64, 9 * 64), (768, 9 * 768), (12, 1)]         # (Cout, K)
FOLD_REL = 2.0 ** -50
# assembled ops.batch_norm_act in eval mode, (N, C, H, W): generic, the padded psi lane, two channel groups
ASSEMBLED = [(2, 8, 9, 7), (1, 1, 5, 5), (2, 260, 6, 6)]


def slope_of(act):
    return SLOPE if act == ACT_LRELU else 0.0


# ============================================================================ data
def frozen_consts(C, seed):
    """(mean, invstd, weight, bias, scale, shift) of a trained layer: |mean| / sigma up to ~10, gamma of both signs, one gamma = 0
    channel; scale = fl(gamma invstd), shift = fl(fma(-mean, scale, beta)) as ops.batch_norm_act's torch ops leave them."""
    rng = np.random.RandomState(seed)
    var = f32(rng.uniform(0.05, 4.0, C))
    mean = f32(rng.uniform(-10, 10, C) * np.sqrt(var))
    w, b = br.affine_data(C, seed + 1)
    w[C // 2] = 0.0
    invstd = f32(1.0 / np.sqrt(var.astype(F64) + 1e-5))
    scale = f32(w * invstd)
    shift = f32(f32(-mean * scale) + b)
    return mean, invstd, w, b, scale, shift


def frozen_x(P, C, mean, invstd, seed):
    """Activations scattered around the running mean with about the running spread (so that pre-activations take both signs)."""
    z = np.random.RandomState(seed).standard_normal((P, C))
    return f32(mean.astype(F64) + z / invstd.astype(F64))


# ============================================================================ references
def grad_ref(x, y_pos, dy, scale, shift, act, slope):
    """(g, dg): the masked gradient as an exact fp64 value and the error granted on it (None for the mask family, where g is an fp32
    value the kernel must reproduce bit for bit)."""
    if act == ACT_SWISH:
        _, zr, mag = br.apply_ref(x, scale, shift, None, ACT_NONE, 0.0)
        gz = 2 * U32 * mag + DENORM
        g = br.masked_grad(dy, None, act, slope, z=zr)
        return g, np.abs(np.asarray(dy, dtype=F64)) * br.swish_grad_gate(zr, gz) + U32 * np.abs(g)
    return br.masked_grad(dy, y_pos, act, slope), None


def dx_gate(g, dg, y_pos, scale, act):
    """(reference, gate) of dx = g * scale (scale None: dx = g, exact for the mask family).  One fp32 rounding of the product; the
    reference multiplies the fp32 g, so LeakyReLU's first rounding is already in it -- measured against fp64 dy slope scale it is
    the one more rounding the negative side is allowed (see dx_gate64)."""
    sc = 1.0 if scale is None else np.asarray(scale, dtype=F64)
    ref = g * sc
    extra = 0.0 if dg is None else np.abs(sc) * dg
    if scale is None:
        return ref, extra * (1 + U32)
    return ref, U32 * (np.abs(ref) + extra) + extra + DENORM


def dx_gate64(dy, y_pos, scale, act, slope):
    """The mask family against the fp64 expression dy act' scale itself: one rounding, two on LeakyReLU's negative side."""
    dy = np.asarray(dy, dtype=F64); sc = np.asarray(scale, dtype=F64)
    if act == ACT_NONE:
        ref = dy * sc; n = 1.0
    else:
        off = 0.0 if act == ACT_RELU else float(F32(slope))
        ref = np.where(y_pos, dy, dy * off) * sc
        n = np.where(y_pos, 1.0, 2.0) if act == ACT_LRELU else 1.0
    return ref, n * U32 * np.abs(ref) * (1 + U32) + DENORM


def frozen_ratios(x, y_pos, dy, mean, invstd, scale, shift, act, slope, dx=None, dres=None, s1=None, s2=None):
    """Error / gate of every output given (pass: <= 1).  x / mean / scale may be None as at the entry point."""
    P, C = np.shape(dy)
    g, dg = grad_ref(x, y_pos, dy, scale, shift, act, slope)
    out = {}
    if dres is not None:
        out['dres'] = (0.0 if same_bits(dres, f32(g)) else float('inf')) if dg is None else worst_ratio(np.asarray(dres, dtype=F64) - g, dg)
    if dx is not None:
        ref, gate = dx_gate(g, dg, y_pos, scale, act)
        if dg is None and scale is None:
            out['dx'] = 0.0 if same_bits(dx, f32(g)) else float('inf')
        else:
            out['dx'] = worst_ratio(np.asarray(dx, dtype=F64) - ref, gate)
        if act == ACT_LRELU and scale is not None:       # (NONE / ReLU: g is dy or a signed zero, the fp64 expression IS g * scale)
            ref64, gate64 = dx_gate64(dy, y_pos, scale, act, slope)
            out['dx64'] = worst_ratio(np.asarray(dx, dtype=F64) - ref64, gate64)
    if s1 is not None:
        a1 = br._colsum(np.abs(g))
        e1 = 0.0 if dg is None else br._colsum(dg)
        out['s1'] = worst_ratio(np.asarray(s1, dtype=F64) - br._colsum(g), br.sum_gate(P, C, a1) + e1)
    if s2 is not None:
        if mean is None:
            out['s2'] = 0.0 if not np.any(np.asarray(s2)) else float('inf')
        else:
            ref = br.bwd_sums_ref(x, g, mean, invstd)
            xh_abs = np.abs((np.asarray(x, dtype=F64) - np.asarray(mean, dtype=F64)) * np.asarray(invstd, dtype=F64))
            e2 = 0.0 if dg is None else br._colsum(dg * xh_abs)
            out['s2'] = worst_ratio(np.asarray(s2, dtype=F64) - ref['s2'], br.sum_gate(P, C, ref['a2'], extra=3) + e2)
    return out


def assembled_ratios(x, y_pos, dy, mean, invstd, scale, shift, act, slope, ref, got):
    """ops.batch_norm_act in eval mode against fp64 autograd through torch.nn.functional.batch_norm(training=False) (`ref`: dict of
    the fp64 gradients dx, dres, dweight, dbias as [P, C] rows / [C]; `got` the same from the HIP path; mean / invstd / scale / shift
    the layer's fp32 constants).  The fp64 function is evaluated at a variance whose rsqrt(var + eps) is the layer's fp32 invstd, so:
    dres     the kernel gate (bits; swish: its derivative's gate);
    dx       the fp64 function multiplies g by gamma invstd, the layer by scale = fl(gamma invstd): one rounding more than the kernel
             gate -- two on |dx|, three on LeakyReLU's negative side;
    dbias    fl32 of the fp64 sum: bn_ref.sum_gate plus one fp32 rounding;  dweight likewise with the 3 roundings inside g xhat;
             LeakyReLU: each negative-side term carries the rounding of dy * slope, u32 |g| per term."""
    P, C = np.shape(dy)
    Cp = (C + 3) // 4 * 4
    g, dg = grad_ref(x, y_pos, dy, scale, shift, act, slope)
    out = {}
    if 'dres' in got:
        # bits of the kernel's contract (dy * 0.f keeps dy's sign on the zero; autograd's where() leaves +0 there) and the value of fp64 autograd
        # (LeakyReLU's dy * slope is one fp32 rounding of the fp64 product)
        out['dres'] = (worst_ratio(np.asarray(got['dres'], dtype=F64) - ref['dres'], U32 * np.abs(ref['dres']) if act == ACT_LRELU else 0.0)
                       if same_bits(got['dres'], f32(g)) else float('inf')) if dg is None else worst_ratio(np.asarray(got['dres'], dtype=F64) - ref['dres'], dg)
    n = np.where(y_pos, 2.0, 3.0) if act == ACT_LRELU else 2.0
    extra = 0.0 if dg is None else np.abs(np.asarray(scale, dtype=F64)) * dg
    out['dx'] = worst_ratio(np.asarray(got['dx'], dtype=F64) - ref['dx'], n * U32 * (np.abs(ref['dx']) + extra) + extra + DENORM)
    if 'dbias' in got:
        xh_abs = np.abs((np.asarray(x, dtype=F64) - np.asarray(mean, dtype=F64)) * np.asarray(invstd, dtype=F64))
        # error of one term against the fp64 function: swish's derivative gate; LeakyReLU's fp32 product dy * slope on the negative side
        # (the fp64 function multiplies exactly, the kernel's g is that product rounded once); none otherwise
        el = dg if dg is not None else (U32 * np.abs(g) * ~np.asarray(y_pos, dtype=bool) if act == ACT_LRELU else None)
        g1 = br.sum_gate(P, Cp, br._colsum(np.abs(g))) + (0.0 if el is None else br._colsum(el))
        g2 = br.sum_gate(P, Cp, br._colsum(np.abs(g) * xh_abs), extra=3) + (0.0 if el is None else br._colsum(el * xh_abs))
        out['dbias'] = worst_ratio(np.asarray(got['dbias'], dtype=F64) - ref['dbias'], g1 + U32 * (np.abs(ref['dbias']) + g1) + DENORM)
        out['dweight'] = worst_ratio(np.asarray(got['dweight'], dtype=F64) - ref['dweight'], g2 + U32 * (np.abs(ref['dweight']) + g2) + DENORM)
    return out


def fold_ref(dwf, w, s, mean, invstd, sums_g):
    """(dw, dgamma, dbeta, gate of dgamma, gate of dbeta): dw the exact fp32 product; dgamma in extended precision on the fp32 inputs."""
    L = np.longdouble
    dwf = f32(dwf); w = f32(w)
    dw = f32(dwf * f32(s)[:, None])
    prod = dwf.astype(L) * w.astype(L)
    t = prod.sum(axis=1)
    mag = np.abs(prod).sum(axis=1).astype(F64) + np.abs(f32(mean).astype(F64) * np.asarray(sums_g, dtype=F64))
    dg = ((t - f32(mean).astype(L) * np.asarray(sums_g, dtype=F64).astype(L)) * f32(invstd).astype(L)).astype(F64)
    inner = FOLD_REL * np.abs(f32(invstd).astype(F64)) * mag
    return dw, dg, np.asarray(sums_g, dtype=F64), U32 * (np.abs(dg) + inner) + inner + DENORM, U32 * np.abs(sums_g) + DENORM


def fold_ratios(dwf, w, s, mean, invstd, sums_g, dw=None, dgamma=None, dbeta=None):
    rw, rg, rb, gg, gb = fold_ref(dwf, w, s, mean, invstd, sums_g)
    out = {}
    if dw is not None:
        out['dw'] = 0.0 if same_bits(dw, rw) else float('inf')
    if dgamma is not None:
        out['dgamma'] = worst_ratio(np.asarray(dgamma, dtype=F64) - rg, gg)
        out['dbeta'] = worst_ratio(np.asarray(dbeta, dtype=F64) - rb, gb)
    return out


def fold_data(Cout, K, seed):
    """(dwf, w, s, mean, invstd, sums_g) with |mean| / sigma up to ~10 and gamma of both signs (so t and mean sum_g cancel)."""
    rng = np.random.RandomState(seed)
    mean, invstd, g, _, s, _ = frozen_consts(Cout, seed + 3)
    dwf = f32(rng.standard_normal((Cout, K)) * 0.1)
    w = f32(rng.standard_normal((Cout, K)) / np.sqrt(K))
    sums_g = rng.standard_normal(Cout) * 30.0
    return dwf, w, s, mean, invstd, sums_g


# ============================================================================ emulations
def frozen_bwd_emul(x, y, dy, mean, invstd, scale, shift, act, slope, mask_from_x=False, dx_no_scale=False, s2_raw_x=False,
                    reduce=True):
    """col_reduce_kernel<3>: (dx, dres, s1, s2).  Planted defects: mask_from_x (the mask is recomputed from x although y was saved --
    wrong wherever the forward added a residual), dx_no_scale (dx = g), s2_raw_x (second sum over x instead of xhat)."""
    yy = None if mask_from_x else y
    xz = x if x is not None else np.zeros_like(f32(dy))
    g = br.masked_grad_emul(xz, yy, dy, scale, shift, act, slope)
    dx = g if (scale is None or dx_no_scale) else f32(g * f32(scale))
    s1 = s2 = None
    if reduce:
        if mean is None:
            s1, _ = br.col_reduce_emul(g.astype(F64), np.zeros(g.shape, F64))
            s2 = np.zeros_like(s1)
        elif s2_raw_x:
            s1, s2 = br.col_reduce_emul(g.astype(F64), g.astype(F64) * f32(x).astype(F64))
        else:
            s1, s2 = br.bwd_reduce_emul(x, g, mean, invstd)
    return dx, g, s1, s2


def fold_bwd_emul(dwf, w, s, mean, invstd, sums_g, no_mean_term=False, dw_unscaled=False):
    """bn_fold_bwd_kernel: thread t adds products k = t, t + 256, ... in fp64, the 256 sums fold in a halving tree."""
    dwf = f32(dwf); w = f32(w)
    Cout, K = dwf.shape
    dw = dwf.copy() if dw_unscaled else f32(dwf * f32(s)[:, None])
    nk = br.cdiv(K, FOLD_BLOCK)
    prod = np.zeros((Cout, nk * FOLD_BLOCK), F64)
    prod[:, :K] = dwf.astype(F64) * w.astype(F64)
    prod = prod.reshape(Cout, nk, FOLD_BLOCK)
    red = np.zeros((Cout, FOLD_BLOCK), F64)
    for i in range(nk):
        red = red + prod[:, i]
    h = FOLD_BLOCK // 2
    while h > 0:
        red = red[:, :h] + red[:, h:2 * h]
        h //= 2
    t = red[:, 0]
    sg = np.asarray(sums_g, dtype=F64)
    inner = t if no_mean_term else t - f32(mean).astype(F64) * sg
    return dw, (inner * f32(invstd).astype(F64)).astype(F32), sg.astype(F32)
