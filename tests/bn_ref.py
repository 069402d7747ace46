"""Plain references for csrc/bn.hip: the two-stage column reductions (batch-norm statistics, the backward's two sums, the plain
channel sum, the fold of conv-epilogue partial rows), bn_finalize_channel, bn_apply and bn_bwd_apply, in fp32 and bf16.  Plain
helper module (not a conftest, no fixtures), numpy and CPU torch only; nothing here calls an op under test.

Four kinds of thing:

* geometry   -- red_geom / the fold rule restated from the host code of bn.hip (tests/test_bn_ref.py pins them to the library's
                host-only workspace queries), and the case lists of tests/test_bn_gpu.py with the geometry fact each case is for;
* *_ref      -- the operation in fp64 (sums with their magnitude sums, two-pass variance, finalize, apply, backward);
* *_emul     -- the kernels' own arithmetic in the kernels' grouping (per-thread strided rows, LDS combine in r order, part rows
                lane-then-row, fold slices), with the planted defects of tests/test_bn_ref.py as keyword switches (all off);
* gates      -- exact, or (rounding count) x (unit roundoff) x (magnitude sum of the reference) per element.  Each count is derived
                beside its gate from bn.hip / common.h; none is fitted."""
from collections import namedtuple
from fractions import Fraction

import numpy as np

from resample_ref import f32, same_bits, worst_ratio  # noqa: F401  (re-exported for the two test files)

U64 = 2.0 ** -53                                # unit roundoff of fp64
U32 = 2.0 ** -24                                # fp32
UBF = 2.0 ** -8                                 # bf16: 8 significand bits (7 stored), so round-to-nearest is within 2^-8 |value| -- not 2^-9:
                                                # 1 + 2^-8 lies midway between the neighbours 1 and 1 + 2^-7 (tests/test_bn_ref.py shows it)
ULP32 = 2.0 ** -23                              # "1 ulp" of a hardware transcendental, as a relative error (common.h)
DENORM = 2.0 ** -149
F32, F64 = np.float32, np.float64
ACT_NONE, ACT_RELU, ACT_LRELU, ACT_SWISH = 0, 1, 2, 3
LOG2E = 1.4426950408889634

RED_BLOCK, MAX_PARTS, FIN_LANES, FOLD_Z, FOLD_LANES = 256, 1024, 32, 64, 8


def cdiv(a, b):
    return -(-a // b)


# ============================================================================ 1. geometry, restated from the host code
RedGeom = namedtuple('RedGeom', 'TQ PR groups parts rows_per_part est CQ')


def red_geom(P, C, Q=1):
    """red_geom of bn.hip.  `est` is the first estimate of parts (after the MAX_PARTS clamp), `CQ` the channel groups of 4 Q."""
    CQ = cdiv(C, 4 * Q)
    TQ = 64 if CQ >= 64 else 1
    if CQ < 64:
        while TQ < CQ:
            TQ <<= 1
    PR = RED_BLOCK // TQ
    groups = cdiv(CQ, TQ)
    est = max(min(cdiv(P, PR * 8), MAX_PARTS), 1)
    rpp = cdiv(P, est)
    return RedGeom(TQ, PR, groups, cdiv(P, rpp), rpp, est, CQ)


def workspace_bytes(P, C):
    """ssg_bn_workspace_bytes: the larger of the fp32 (Q = 1) and bf16 (Q = 2) partial-row buffers."""
    return max(red_geom(P, C, q).parts * 2 * 4 * q * cdiv(C, 4 * q) * 8 for q in (1, 2))


def fold_geom(rows):
    """(fold?, rpz, nz) of ssg_bn_stats_from_partials_*: rows > 4 FOLD_Z are first folded in nz slices of rpz rows."""
    if rows <= 4 * FOLD_Z:
        return False, rows, 1
    rpz = cdiv(rows, FOLD_Z)
    return True, rpz, cdiv(rows, rpz)


def partials_workspace_bytes(rows, C):
    return FOLD_Z * 2 * C * 8 if rows > 4 * FOLD_Z else 16


def live_lanes_last_group(g):
    return g.CQ - (g.groups - 1) * g.TQ


# ============================================================================ 2. case lists (P, C, facts the case exists for)
_CS32 = [4, 8, 12, 16, 32, 40, 64, 128, 256, 260, 384]


def first_shrinking_p(C, Q=1):
    """Smallest P whose recomputed parts is below the first estimate.  Unclamped, est = ceil(P / 8 PR) gives rows_per_part <= 8 PR
    and P > 8 PR (est - 1), so ceil(P / rows_per_part) = est: parts shrink only once MAX_PARTS clamps the estimate."""
    P = 1
    while True:
        g = red_geom(P, C, Q)
        if g.parts < g.est:
            return P
        P += 1


def _stat_cases_f32():
    cases = []
    for k in range(1, 32):                               # parts = 1..31 (second stage: that many live lanes), C cycling over every TQ
        C = _CS32[(k - 1) % len(_CS32)]
        PR = red_geom(1, C).PR
        cases.append((PR * 8 * k - 1, C, dict(parts=k, short_last=True) if k > 1 else dict(parts=1)))
    cases += [
        (1, 4, dict(parts=1, TQ=1, P_lt_PR=True)),
        (1, 260, dict(parts=1, groups=2, live_last=1)),
        (3, 4, dict(P_lt_PR=True, TQ=1)),
        (2, 256, dict(P_lt_PR=True, TQ=64, groups=1)),
        (1021, 256, dict(parts=32)),                     # a multiple of FIN_LANES
        (2045, 256, dict(parts=64)),
        (1053, 256, dict(parts=33)),                     # > 32, no multiple
        (1437, 256, dict(parts=45)),
        (32768 + 5, 256, dict(clamp=True, TQ=64, shrinks=True, parts=994)),      # parts shrink only under the clamp (see below)
        ((1 << 21) + 3, 4, dict(clamp=True, TQ=1, parts=1024)),
    ]
    return cases


def _stat_cases_bf16():
    return [
        (1, 8, dict(parts=1, TQ=1, P_lt_PR=True)),
        (5, 24, dict(TQ=4, idle_lanes=True, P_lt_PR=True)),
        (64 * 8 * 2 - 1, 24, dict(parts=2, short_last=True, idle_lanes=True)),
        (4 * 8 * 3 - 1, 512, dict(parts=3, TQ=64, groups=1, short_last=True)),
        (4 * 8 * 5 - 1, 520, dict(parts=5, groups=2, live_last=1, short_last=True)),
        (4 * 8 * 32 - 3, 512, dict(parts=32)),
        (256 * 8 * 33 - 3, 8, dict(parts=33, TQ=1)),
        (32768 + 5, 512, dict(clamp=True, TQ=64, shrinks=True, parts=994)),
    ]


STAT_CASES_F32 = _stat_cases_f32()
STAT_CASES_BF16 = _stat_cases_bf16()
CHANNEL_SUM_EXTRA = [(517, 6), (33, 1), (285, 258)]     # ssg_channel_sum_f32 alone takes C % 4 != 0
PARTIAL_CASES = [(r, c) for r in (1, 31, 33, 256, 257, 300, 4097) for c in (4, 40, 64)]
LDS_CASES = [(7, 1228, False), (5, 1232, True), (3, 2688, True), (2, 4096, True)]        # (P, C, dynamic-LDS opt-in expected)
LDS_CASES_BF16 = [(7, 1224, False)] + LDS_CASES[1:]     # C % 8 == 0: 1224 is the last bf16 size inside 48 KiB
BIG = 1 << 22                                            # elements from which a case runs a shortened list of activation plans
LDS_REFUSED_C = 4100
LD_CASE = (285, 40, 56)                                  # (P, C, ld): a channel slice of a wider NHWC tensor
LD_CASE_STRIDES = dict(x=56, y=48, dy=64, dx=72, dres=80)    # the slice test's row strides, all distinct (multiples of 8 for bf16)
# backward: MODE 1 is its own instantiation (mask, xhat): the same geometry lists as the statistics
BWD_CASES_F32 = STAT_CASES_F32
BWD_CASES_BF16 = STAT_CASES_BF16


def check_facts(P, C, Q, facts):
    """The geometry facts a case claims, against the restated red_geom.  Returns the list of violated claims."""
    g = red_geom(P, C, Q)
    bad = []
    for k, v in facts.items():
        if k in ('parts', 'TQ', 'groups'):
            ok = getattr(g, k) == v
        elif k == 'short_last':
            ok = g.parts >= 2 and P % g.rows_per_part != 0
        elif k == 'P_lt_PR':
            ok = P < g.PR
        elif k == 'live_last':
            ok = live_lanes_last_group(g) == v
        elif k == 'idle_lanes':
            ok = live_lanes_last_group(g) < g.TQ
        elif k == 'shrinks':
            ok = g.parts < g.est
        elif k == 'clamp':
            ok = cdiv(P, g.PR * 8) > MAX_PARTS and g.est == MAX_PARTS
        else:
            ok = False
        if not ok:
            bad.append((k, v, g))
    return bad


# ============================================================================ 3. data
def bf16_rne(a):
    """fp32 -> the nearest bf16 (ties to even), returned as fp32.  Finite inputs."""
    u = f32(a).view(np.uint32)
    return ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)).view(np.float32)


def bf16_trunc(a):
    return (f32(a).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


N_KINDS = 6


def stats_data(P, C, seed, bf16=False):
    """[P, C] fp32, channel c of kind c % 6:
    0 mean 0 std 1 | 1 mean 1e3 std 1e-2 (mean^2 / var = 1e10; var 1e-4 lies between the two eps) | 2 the constant 0.1f (var 0,
    s2/n - m^2 may come out negative) | 3 all zero | 4 mean 0.5 std 5e-4 (var 2.5e-7 < eps, mean/std = 1e3) | 5 mean -2 std 0.3."""
    rng = np.random.RandomState(seed)
    z = rng.standard_normal((P, C))
    kind = np.arange(C) % N_KINDS
    mean = np.choose(kind, [0.0, 1e3, 0.1, 0.0, 0.5, -2.0])
    std = np.choose(kind, [1.0, 1e-2, 0.0, 0.0, 5e-4, 0.3])
    x = f32(mean + std * z)
    return bf16_rne(x) if bf16 else x


def grad_data(P, C, seed, bf16=False):
    g = f32(np.random.RandomState(seed).standard_normal((P, C)))
    return bf16_rne(g) if bf16 else g


def affine_data(C, seed):
    rng = np.random.RandomState(seed)
    return f32(rng.uniform(0.5, 1.5, C) * np.where(rng.rand(C) < 0.25, -1, 1)), f32(rng.standard_normal(C) * 0.3)


def bwd_consts(x, C, seed, eps=1e-5, var_mode=0, affine=True):
    """The fp32 constants a backward test hands to the kernels: (weight, bias, mean, invstd, scale, shift) from the fp64 statistics
    of x, each rounded to fp32 (scale and shift formed from the rounded ones, as the forward leaves them)."""
    ref = stats_ref(x)
    w, b = affine_data(C, seed) if affine else (None, None)
    mean = f32(ref['mean']); invstd = f32(invstd_of(ref['var'], float(F32(eps)), var_mode))
    fin = finalize_exact(mean, invstd, w, b, 0.1, None)
    return w, b, mean, invstd, fin['scale'], fin['shift']


def partial_rows(rows, C, seed):
    """[rows][2][C] fp64 with magnitudes spread over 1e12 (row r scaled by 10^(12 (r*7 % 13) / 12)), so that the order of the
    additions matters; s2 rows non-negative like sums of squares."""
    rng = np.random.RandomState(seed)
    part = rng.standard_normal((rows, 2, C))
    part[:, 1] = np.abs(part[:, 1])
    part *= (10.0 ** ((np.arange(rows) * 7 % 13)))[:, None, None]
    return np.ascontiguousarray(part)


def mask_probe(C, per_channel, seed, bf16=False):
    """x [P, C] whose every pre-activation x*scale + shift is within rounding of 0: for random (scale, shift) per channel the
    neighbours, within +-4 ulp (of the storage type), of -shift/scale.  Returns (x, scale, shift)."""
    rng = np.random.RandomState(seed)
    scale = f32(rng.uniform(0.25, 4.0, C) * np.where(rng.rand(C) < 0.5, -1, 1))
    shift = f32(rng.uniform(0.25, 4.0, C) * np.where(rng.rand(C) < 0.5, -1, 1))
    x0 = f32(-shift.astype(F64) / scale.astype(F64))
    if bf16:                                            # a bf16 x is 2^16 times coarser than the fp32 product's rounding: take the shift
        x0 = bf16_rne(x0)                               # whose root IS a bf16 value to within that rounding (still random pairs)
        shift = f32(-x0.astype(F64) * scale.astype(F64))
    step = np.tile(np.arange(-4, 5), cdiv(per_channel, 9))[:per_channel]
    bits = x0.view(np.int32)[None, :] + (step[:, None] * (1 << 16 if bf16 else 1)).astype(np.int32)
    return np.ascontiguousarray(bits.astype(np.int32)).view(np.float32), scale, shift


# ============================================================================ exact helpers
def _round_f32(fr):
    """The fp32 nearest to the rational fr (ties to even): one rounding, no double rounding through fp64."""
    c = F32(float(fr))
    best = None
    for cand in (np.nextafter(c, F32(-np.inf)), c, np.nextafter(c, F32(np.inf))):
        if not np.isfinite(cand):
            continue
        d = abs(fr - Fraction(float(cand)))
        even = (int(np.array(cand).view(np.int32)) & 1) == 0
        if best is None or d < best[0] or (d == best[0] and even):
            best = (d, cand)
    return best[1]


def fma32(a, b, c):
    return _round_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def fma64(a, b, c):
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))       # Fraction -> float rounds correctly


def _colsum(a):
    """Column sums accumulated in long double (64 significand bits on x86) and rounded once to fp64: the reference's own error
    is that one rounding, which sum_gate counts as the +1 of its K."""
    return np.asarray(a).sum(axis=0, dtype=np.longdouble).astype(F64)


# ============================================================================ 4. references in fp64
def stats_ref(x):
    """s1, s2, the magnitude sums a1 = sum |x|, a2 = sum x^2, mean and the two-pass biased variance, per channel."""
    x = np.asarray(x, dtype=F64)
    n = x.shape[0]
    s1 = _colsum(x)
    mean = s1 / n
    s2 = _colsum(x * x)
    return dict(s1=s1, s2=s2, a1=_colsum(np.abs(x)), a2=s2, mean=mean, var=_colsum((x - mean) ** 2) / n, count=float(n))


def invstd_of(var, eps, var_mode):
    var = np.asarray(var, dtype=F64)
    return 1.0 / np.sqrt(var + eps) if var_mode == 0 else 1.0 / np.sqrt(np.maximum(var, eps))


def finalize_ref(mean, var, count, weight, bias, eps, momentum, var_mode, running_mean=None, running_var=None):
    """fp64: invstd per var_mode (0: (var + eps)^-1/2, 1: clamp(var, eps)^-1/2), scale = w invstd, shift = b - mean scale, the
    running estimates with the unbiased variance var count / (count - 1) (var itself when count == 1)."""
    eps = float(F32(eps)); momentum = float(F32(momentum))
    mean = np.asarray(mean, dtype=F64); var = np.asarray(var, dtype=F64)
    w = np.ones_like(mean) if weight is None else np.asarray(weight, dtype=F64)
    b = np.zeros_like(mean) if bias is None else np.asarray(bias, dtype=F64)
    invstd = invstd_of(var, eps, var_mode)
    out = dict(mean=mean, invstd=invstd, scale=w * invstd, shift=b - mean * w * invstd)
    if running_mean is not None:
        out['running_mean'] = momentum * mean + (1 - momentum) * np.asarray(running_mean, dtype=F64)
    if running_var is not None:
        unb = var * count / (count - 1) if count > 1 else var
        out['running_var'] = momentum * unb + (1 - momentum) * np.asarray(running_var, dtype=F64)
    return out


def sigmoid64(z):
    z = np.asarray(z, dtype=F64)
    with np.errstate(over='ignore'):
        return np.where(z >= 0, 1.0 / (1.0 + np.exp(-np.abs(z))), np.exp(-np.abs(z)) / (1.0 + np.exp(-np.abs(z))))


def swish_grad64(z):
    s = sigmoid64(z)
    return s * (1.0 + z * (1.0 - s))


def act64(z, act, slope):
    if act == ACT_RELU:
        return np.where(z < 0, 0.0, z)
    if act == ACT_LRELU:
        return np.where(z > 0, z, z * float(F32(slope)))
    if act == ACT_SWISH:
        return z * sigmoid64(z)
    return z


def apply_ref(x, scale, shift, res, act, slope):
    """(y, z, mag): y = act(z), z = x scale + shift (+ res) in fp64, mag = |x scale| + |shift| (+ |res|)."""
    x = np.asarray(x, dtype=F64); sc = np.asarray(scale, dtype=F64); sh = np.asarray(shift, dtype=F64)
    z = x * sc + sh
    mag = np.abs(x * sc) + np.abs(sh)
    if res is not None:
        z = z + np.asarray(res, dtype=F64); mag = mag + np.abs(np.asarray(res, dtype=F64))
    return act64(z, act, slope), z, mag


def masked_grad(dy, y_mask_pos, act, slope, z=None, bf16=False):
    """g = dy act' as the kernels form it.  ReLU / LeakyReLU: dy where the forward output is > 0 (`y_mask_pos`, the kernel's
    contract), else the fp32 product dy * 0 (a signed zero) or dy * slope -- an fp32 value, exact.  Swish: fp64 dy * swish'(z).  None: dy."""
    dy = f32(dy)
    if act == ACT_NONE:
        return dy.astype(F64)
    if act == ACT_SWISH:
        return dy.astype(F64) * swish_grad64(z)
    off = dy * (F32(0) if act == ACT_RELU else F32(slope))          # `g *= 0.f` keeps dy's sign on the zero
    return np.where(y_mask_pos, dy, off).astype(F64)


def bwd_sums_ref(x, g, mean, invstd):
    """s1 = sum g, s2 = sum g xhat, with their magnitude sums, xhat = (x - mean) invstd from the fp32 constants handed to the kernel."""
    x = np.asarray(x, dtype=F64); g = np.asarray(g, dtype=F64)
    xh = (x - np.asarray(mean, dtype=F64)) * np.asarray(invstd, dtype=F64)
    return dict(s1=_colsum(g), s2=_colsum(g * xh), a1=_colsum(np.abs(g)), a2=_colsum(np.abs(g * xh)))


def dx_ref(x, g, mean, invstd, weight, s1, s2, count):
    """(dx, mag): dx = w invstd (g - m1 - xhat m2), mag = w invstd (|g| + |m1| + |xhat m2|), m1 = s1 / count, m2 = s2 / count."""
    x = np.asarray(x, dtype=F64); g = np.asarray(g, dtype=F64)
    mu = np.asarray(mean, dtype=F64); is_ = np.asarray(invstd, dtype=F64)
    w = np.ones_like(mu) if weight is None else np.asarray(weight, dtype=F64)
    m1 = np.asarray(s1, dtype=F64) / count; m2 = np.asarray(s2, dtype=F64) / count
    xh = (x - mu) * is_
    return w * is_ * (g - m1 - xh * m2), np.abs(w * is_) * (np.abs(g) + np.abs(m1) + np.abs(xh * m2))


# ============================================================================ 5. gates
def k_sum(P, C, Q=1):
    """Longest chain of fp64 additions a value passes through in run_reduce: the rows one thread adds (ceil(rows_per_part / PR)),
    the PR rows of the LDS combine, the ceil(parts / 32) part rows of one lane of col_reduce_final_kernel, its 32 lanes."""
    g = red_geom(P, C, Q)
    return cdiv(g.rows_per_part, g.PR) + g.PR + cdiv(g.parts, FIN_LANES) + FIN_LANES


def k_thread(P, C, Q=1):
    g = red_geom(P, C, Q)
    return cdiv(g.rows_per_part, g.PR)


def k_partials(rows):
    """fold (rows > 256): ceil(rpz / 8) rows of a row-lane, its 8 lanes, then ceil(nz / 32) + 32 of the final stage; else
    ceil(rows / 32) + 32."""
    fold, rpz, nz = fold_geom(rows)
    return (cdiv(rpz, FOLD_LANES) + FOLD_LANES + cdiv(nz, FIN_LANES) + FIN_LANES) if fold else (cdiv(rows, FIN_LANES) + FIN_LANES)


def sum_gate(P, C, mag, bf16=False, extra=0):
    """Gate of a column sum.  fp32 tensors: every addition is fp64, K = k_sum (+ `extra` roundings inside one term: the backward's
    xhat = (x - mean) invstd and g xhat are three).  bf16 tensors: the k_thread additions of one thread (and the `extra` term
    roundings) are fp32, the k_sum - k_thread cross-thread ones fp64."""
    return sum_rel(P, C, bf16, extra) * np.asarray(mag, dtype=F64)


def sum_rel(P, C, bf16=False, extra=0):
    """The factor of sum_gate; the + 1 is the reference's own rounding to fp64 (_colsum)."""
    if bf16:
        return (k_thread(P, C, 2) + extra) * U32 + (k_sum(P, C, 2) - k_thread(P, C, 2) + 1) * U64
    return (k_sum(P, C) + extra + 1) * U64


def moment_gates(ref, K_rel, eps, var_mode):
    """Gates of the fp32 mean and invstd that bn_finalize_channel forms from sums with relative-to-magnitude error K_rel (that is
    |s1 - S1| <= K_rel a1, |s2 - S2| <= K_rel a2):
    mean  : one fp32 rounding, plus dm = (K_rel + u64) a1 / count (the sum, the division);
    var   : s2 / count (the sum, the division), the fma's own rounding, and m^2 moved by dm: dv = (K_rel + 2 u64) a2 / count + 2 |m| dm + dm^2;
    invstd: one fp32 rounding of f(var), f evaluated over [var - dv, var + dv] (clamped at 0 as the kernel clamps) -- f is monotone,
            so the ends bound it -- plus 4 u64 for sqrt, +eps, division."""
    n = ref['count']
    eps = float(F32(eps))
    dm = (K_rel + U64) * ref['a1'] / n
    dv = (K_rel + 2 * U64) * ref['a2'] / n + 2 * np.abs(ref['mean']) * dm + dm * dm
    f0 = invstd_of(ref['var'], eps, var_mode)
    lo = invstd_of(np.maximum(ref['var'] - dv, 0.0), eps, var_mode); hi = invstd_of(ref['var'] + dv, eps, var_mode)
    spread = np.maximum(np.abs(lo - f0), np.abs(hi - f0))
    return dict(mean=U32 * np.abs(ref['mean']) + dm + DENORM, invstd=U32 * (f0 + spread) + spread + 4 * U64 * f0, var=dv)


def finalize_exact(mean, invstd, weight, bias, momentum, running_mean):
    """scale, shift, running_mean as the specified function of the kernel's own fp32 mean / invstd: sc = fl(w is),
    shift = fma(-mean, sc, b), running_mean = fma(momentum, mean, fl(fl(1 - momentum) rm)); exact rational arithmetic, one rounding each."""
    mean = f32(mean); invstd = f32(invstd); C = mean.size
    w = np.ones(C, F32) if weight is None else f32(weight); b = np.zeros(C, F32) if bias is None else f32(bias)
    sc = (w.astype(F64) * invstd.astype(F64)).astype(F32)                  # a 48-bit product is exact in fp64: one rounding
    out = dict(scale=sc, shift=np.array([fma32(-mean[c], sc[c], b[c]) for c in range(C)], dtype=F32))
    if running_mean is not None:
        keep = (F32(1) - F32(momentum)) * f32(running_mean)
        out['running_mean'] = np.array([fma32(F32(momentum), mean[c], keep[c]) for c in range(C)], dtype=F32)
    return out


def running_var_exact(s1, s2, count, momentum, running_var, no_unbias=False):
    """running_var as the specified function of the fp64 sums: m = s1 / n, var = max(fma(-m, m, s2 / n), 0),
    unb = var n / (n - 1) (n > 1), fma(momentum, (float) unb, fl(fl(1 - momentum) rv))."""
    s1 = np.asarray(s1, dtype=F64); s2 = np.asarray(s2, dtype=F64); n = F64(count)
    m = s1 / n; q = s2 / n
    var = np.maximum(np.array([fma64(-m[c], m[c], q[c]) for c in range(m.size)]), 0.0)
    unb = var * n / (n - 1) if (count > 1 and not no_unbias) else var
    keep = (F32(1) - F32(momentum)) * f32(running_var)
    return np.array([fma32(F32(momentum), F32(unb[c]), keep[c]) for c in range(m.size)], dtype=F32), var


def apply_gate(mag, y_ref, z_ref, act, res, bf16=False):
    """fp32: two roundings over |x scale| + |shift| (product and sum; one if contracted), a third with a residual.  ReLU exact after
    that (1-Lipschitz); LeakyReLU's v * slope is one more rounding of the result.  Swish: see swish_gate.  bf16: + 2^-8 |y| for the store."""
    gz = (3 if res else 2) * U32 * mag + DENORM
    if act == ACT_SWISH:
        g = swish_gate(z_ref, gz)
    elif act == ACT_LRELU:
        # only the negative side rounds: |v slope| <= |y_ref| + gz where z_ref <= 0, and <= gz where the kernel's v <= 0 < z_ref
        g = gz + U32 * (np.where(np.asarray(z_ref) <= 0, np.abs(y_ref), 0.0) + gz)
    else:
        g = gz
    return g + (UBF * (np.abs(y_ref) + g) if bf16 else 0.0)


def sigmoid_rel(z):
    """Relative error of ssg_sigmoid_fast(z) = rcp(1 + __expf(-z)), from the 1-ulp figures of common.h:
    __expf(-z) = v_exp_f32(-z log2e): the argument carries two roundings (the constant, the product), each amplified to
    |z| log2e u32 in the result; v_exp_f32 itself 1 ulp: e_e = 2^-23 + 2 |z| log2e u32.  1 + e: e's error reaches the sum as
    e e_e / (1 + e) = (1 - sigma) e_e, the addition rounds (u32); v_rcp_f32 1 ulp."""
    z = np.asarray(z, dtype=F64)
    e_e = ULP32 + 2 * np.abs(z) * LOG2E * U32
    return (1 - sigmoid64(z)) * e_e + U32 + ULP32


SWISH_LIP = 1.1            # sup |swish'| = 1.0998 (at z = 2.3994)


def swish_gate(z, gz):
    """|y - z sigma(z)|: the pre-activation's error gz through |swish'| <= 1.1, sigma's relative error and the product's rounding on |y|."""
    z = np.asarray(z, dtype=F64)
    return SWISH_LIP * gz + np.abs(z * sigmoid64(z)) * (sigmoid_rel(z) + U32) + DENORM


SWISH_GRAD_LIP = 0.5       # sup |swish''| = 0.5 (at z = 0)


def swish_grad_gate(z, gz):
    """|d - swish'(z)| for d = s (1 + z (1 - s)), s = sigma(z)(1 + e_s):
    a = 1 - s      : da = s e_s + u32 (1 - s)
    b = z a        : db = |z| da + u32 |z (1 - s)|        (none if contracted into the next line's fma)
    c = 1 + b      : dc = db + u32 |1 + z (1 - s)|
    d = s c        : dd = s dc + s e_s |c| + u32 |d|
    plus the pre-activation's error gz through |swish''| <= 0.5."""
    z = np.asarray(z, dtype=F64)
    s = sigmoid64(z); es = sigmoid_rel(z)
    da = s * es + U32 * (1 - s)
    db = np.abs(z) * da + U32 * np.abs(z * (1 - s))
    c = 1 + z * (1 - s)
    dc = db + U32 * np.abs(c)
    return s * dc + s * es * np.abs(c) + U32 * np.abs(s * c) + SWISH_GRAD_LIP * gz + DENORM


def swish_limit_ok(z, y, d, u=0.0):
    """|z| >= 20: only the limits.  z > 0: y -> z and swish' -> 1 (within z e^-z, (1 + z) e^-z and a few fp32 roundings);
    z < 0: y -> -0 from below (sign bit set, |y| <= |z| e^-|z|) and swish' -> 0.  All finite.  u: the store's unit roundoff (bf16)."""
    y = float(y); d = float(d); a = abs(float(z))
    tail = float(np.exp(-a)) * (1.001 + u)
    if not (np.isfinite(y) and np.isfinite(d)):
        return False
    if z > 0:
        return abs(y - z) <= a * (tail + 2 * ULP32 + u) and abs(d - 1) <= (1 + a) * tail + 3 * ULP32 + u
    return bool(np.signbit(y)) and abs(y) <= a * tail and abs(d) <= (1 + a) * tail + DENORM


K_DX = 8


def dx_gate(dx, mag, bf16=False, dg=None, w_is=None):
    """bn_bwd_apply's dx = k_ws ((acc) g - k_m1 - xh k_m2), xh = ((acc) x - k_mean) k_is.  Roundings in the accumulation type on the
    way of a term to the result: k_ws (1), k_m1 or k_m2 (1 each, the division), xh's subtraction and product (2), xh k_m2 (1), the
    two subtractions (2), the product with k_ws (1): 8 at most, relative to mag = w invstd (|g| + |m1| + |xh m2|).
    fp32 tensors: acc = fp64, then ONE fp32 rounding of the result.  bf16 tensors: acc = fp32, then one bf16 rounding.
    dg: error of g itself (swish only), reaching dx through w invstd."""
    extra = 0.0 if dg is None else np.abs(w_is) * dg
    if bf16:
        inner = K_DX * U32 * mag + extra
        return UBF * (np.abs(dx) + inner) + inner + DENORM
    inner = K_DX * U64 * mag + extra
    return U32 * (np.abs(dx) + inner) + inner + DENORM


# ============================================================================ 6. emulations
def _lane_sum(rows, lanes):
    """rows [n, ...] fp64: lane l adds rows l, l + lanes, ... in order, then the lanes are added in order (from 0.0)."""
    n = rows.shape[0]
    nb = cdiv(n, lanes)
    pad = np.zeros((nb * lanes,) + rows.shape[1:], dtype=F64)
    pad[:n] = rows
    pad = pad.reshape((nb, lanes) + rows.shape[1:])
    lane = np.zeros(pad.shape[1:], dtype=F64)
    for i in range(nb):
        lane = lane + pad[i]
    tot = np.zeros(rows.shape[1:], dtype=F64)
    for k in range(lanes):
        tot = tot + lane[k]
    return tot


def col_reduce_emul(t1, t2, Q=1, acc=F64, drop_short_last=False, idle_lane=False):
    """col_reduce_kernel + col_reduce_final_kernel over per-element terms t1, t2 [P, C] (already in the accumulation type):
    thread (pr, channel) adds rows p0 + pr, p0 + pr + PR, ... of its part in `acc`; the PR rows of a block are added in fp64 in r
    order; the part rows lane-then-row.  Planted defects: drop_short_last (a part shorter than rows_per_part is skipped),
    idle_lane (the idle quad lanes of the last group accumulate the group's first channels once more -- no `cok` guard, wrapped
    index -- and the combine adds their LDS rows)."""
    P, C = t1.shape
    g = red_geom(P, C, Q)
    V = 4 * Q
    nit = cdiv(g.rows_per_part, g.PR)
    out = []
    for t in (t1, t2):
        t = np.ascontiguousarray(t, dtype=acc)
        thr = np.zeros((g.parts, g.PR, C), dtype=acc)
        base = (np.arange(g.parts) * g.rows_per_part)[:, None]
        p1 = np.minimum(base + g.rows_per_part, P)
        for i in range(nit):
            off = i * g.PR + np.arange(g.PR)[None, :]
            idx = base + off
            ok = (off < g.rows_per_part) & (idx < p1)
            thr = thr + np.where(ok[:, :, None], t[np.minimum(idx, P - 1)], acc(0))
            assert thr.dtype == acc
        if drop_short_last and P % g.rows_per_part:
            thr[-1] = 0
        thr = thr.astype(F64)
        rows = np.zeros((g.parts, C), dtype=F64)
        for r in range(g.PR):
            rows = rows + thr[:, r]
        if idle_lane and live_lanes_last_group(g) < g.TQ:
            c0 = (g.groups - 1) * g.TQ * V
            rows[:, c0:c0 + V] = rows[:, c0:c0 + V] + rows[:, c0:c0 + V]
        out.append(_lane_sum(rows, FIN_LANES))
    return out[0], out[1]


def stats_emul(x, bf16=False, s2_f32=False, **defects):
    """MODE 0: (sum x, sum x^2).  fp32 tensors accumulate in fp64 (x^2 exact), bf16 tensors in fp32 per thread (the square of a bf16
    value is exact in fp32).  Planted defect s2_f32: the fp32 tensor's squares formed and accumulated in fp32."""
    x = f32(x)
    if bf16:
        return col_reduce_emul(x, x * x, Q=2, acc=F32, **defects)
    if s2_f32:
        a, _ = col_reduce_emul(x.astype(F64), x.astype(F64), **defects)
        _, b = col_reduce_emul(x, x * x, acc=F32, **defects)
        return a, b
    x = x.astype(F64)
    return col_reduce_emul(x, x * x, **defects)


def preact_emul(x, scale, shift, muladd=False):
    """x * scale + shift in fp32: contracted to one fma (the 48-bit product is exact in fp64; the fp64 sum is exact wherever it
    cancels, which is where the sign is decided), or -- muladd -- product rounded, then the sum."""
    x = f32(x)
    if muladd:
        return x * f32(scale) + f32(shift)
    return (x.astype(F64) * f32(scale).astype(F64) + f32(shift).astype(F64)).astype(F32)


def sigmoid_emul(z):
    z = f32(z)
    with np.errstate(over='ignore'):
        return F32(1) / (F32(1) + np.exp(-z))


def swish_grad_emul(z):
    s = sigmoid_emul(z)
    return s * (F32(1) + f32(z) * (F32(1) - s))


def apply_emul(x, scale, shift, res, act, slope, bf16=False, truncate=False):
    """bn_apply_kernel in fp32.  Planted defect truncate: the bf16 store drops the low 16 bits instead of rounding to nearest even."""
    v = preact_emul(x, scale, shift)
    if res is not None:
        v = v + f32(res)
    if act == ACT_RELU:
        v = np.where(v < 0, F32(0), v)
    elif act == ACT_LRELU:
        v = np.where(v > 0, v, v * F32(slope))
    elif act == ACT_SWISH:
        v = v * sigmoid_emul(v)
    v = f32(v)
    return (bf16_trunc(v) if truncate else bf16_rne(v)) if bf16 else v


def masked_grad_emul(x, y, dy, scale, shift, act, slope, mask_muladd=False):
    """g = dy act' in fp32 as col_reduce_kernel<1> and bn_bwd_apply_kernel form it: mask from y when given, else recomputed.
    Planted defect mask_muladd: the recomputed pre-activation is mul + add where the forward used one fma."""
    g = f32(dy).copy()
    if act == ACT_SWISH:
        return f32(g * swish_grad_emul(preact_emul(x, scale, shift)))
    if act != ACT_NONE:
        yv = f32(y) if y is not None else preact_emul(x, scale, shift, muladd=mask_muladd)
        g = np.where(yv > 0, g, g * (F32(0) if act == ACT_RELU else F32(slope)))
    return f32(g)


def bwd_reduce_emul(x, g, mean, invstd, bf16=False, **defects):
    """MODE 1 over the masked g: s1 += g, s2 += g * xh, xh = ((acc) x - mean) * invstd, acc = fp64 (fp32 tensors) or fp32 (bf16)."""
    acc = F32 if bf16 else F64
    xh = (f32(x).astype(acc) - f32(mean).astype(acc)) * f32(invstd).astype(acc)
    ga = f32(g).astype(acc)
    return col_reduce_emul(ga, ga * xh, Q=2 if bf16 else 1, acc=acc, **defects)


def bwd_apply_emul(x, g, mean, invstd, weight, s1, s2, count, bf16=False, consts_f32=False, truncate=False):
    """bn_bwd_apply_kernel's dx.  Planted defects: consts_f32 (m1, m2, w invstd of an fp32 tensor rounded to fp32), truncate (bf16 store)."""
    acc = F32 if bf16 else F64
    is64 = f32(invstd).astype(F64)
    w64 = np.ones_like(is64) if weight is None else f32(weight).astype(F64)
    kws = w64 * is64; m1 = np.asarray(s1, dtype=F64) / F64(count); m2 = np.asarray(s2, dtype=F64) / F64(count)
    if consts_f32:
        kws, m1, m2 = (a.astype(F32).astype(F64) for a in (kws, m1, m2))
    kws, m1, m2 = kws.astype(acc), m1.astype(acc), m2.astype(acc)
    xh = (f32(x).astype(acc) - f32(mean).astype(acc)) * f32(invstd).astype(acc)
    o = kws * (f32(g).astype(acc) - m1 - xh * m2)
    assert o.dtype == acc
    o = o.astype(F32)
    return (bf16_trunc(o) if truncate else bf16_rne(o)) if bf16 else o


def partials_emul(part, drop_tail=False):
    """ssg_bn_stats_from_partials_*: rows > 256 are folded in nz slices (8 row-lanes each, rows of a lane in order, lanes in order),
    then col_reduce_final_kernel's lane-then-row sum.  Planted defect drop_tail: nz = floor(rows / rpz), the rows beyond nz rpz dropped."""
    part = np.asarray(part, dtype=F64)
    rows = part.shape[0]
    fold, rpz, nz = fold_geom(rows)
    if fold:
        if drop_tail:
            nz = rows // rpz
        part = np.stack([_lane_sum(part[z * rpz:min((z + 1) * rpz, rows)], FOLD_LANES) for z in range(nz)])
    tot = _lane_sum(part, FIN_LANES)
    return tot[0], tot[1]


def finalize_emul(s1, s2, count, weight, bias, eps, momentum, var_mode, running_mean=None, running_var=None,
                  no_unbias=False, swap_var_mode=False):
    """bn_finalize_channel, every fma spelled as there.  Planted defects: no_unbias (running_var from the biased variance),
    swap_var_mode (var_mode 0 and 1 exchanged).  (Defect 11, the count taken as P instead of sums[2C], is the caller passing the wrong count.)"""
    if swap_var_mode:
        var_mode = 1 - var_mode
    s1 = np.asarray(s1, dtype=F64); s2 = np.asarray(s2, dtype=F64); n = F64(count)
    C = s1.size
    eps64 = F64(F32(eps))
    w = np.ones(C, F32) if weight is None else f32(weight); b = np.zeros(C, F32) if bias is None else f32(bias)
    out = {}
    if running_var is not None:
        out['running_var'], var = running_var_exact(s1, s2, count, momentum, running_var, no_unbias)
    else:
        m = s1 / n; q = s2 / n
        var = np.maximum(np.array([fma64(-m[c], m[c], q[c]) for c in range(C)]), 0.0)
    is_ = 1.0 / np.sqrt(var + eps64) if var_mode == 0 else 1.0 / np.sqrt(np.where(var < eps64, eps64, var))
    out['mean'] = (s1 / n).astype(F32); out['invstd'] = is_.astype(F32)
    out.update(finalize_exact(out['mean'], out['invstd'], w, b, momentum, running_mean))
    return out


# ============================================================================ 7. the gates, as error / gate ratios (pass: <= 1)
def _d(a):
    return np.asarray(a, dtype=F64)


def stats_ratios(x, s1, s2, bf16=False, ref=None):
    P, C = np.shape(x)
    ref = ref or stats_ref(x)
    return {'s1': worst_ratio(_d(s1) - ref['s1'], sum_gate(P, C, ref['a1'], bf16)),
            's2': worst_ratio(_d(s2) - ref['s2'], sum_gate(P, C, ref['a2'], bf16))}


def moment_ratios(ref, mean, invstd, K_rel, eps, var_mode):
    g = moment_gates(ref, K_rel, eps, var_mode)
    return {'mean': worst_ratio(_d(mean) - ref['mean'], g['mean']),
            'invstd': worst_ratio(_d(invstd) - invstd_of(ref['var'], float(F32(eps)), var_mode), g['invstd'])}


def exact_ratios(got, mean, invstd, weight, bias, momentum, running_mean):
    """scale / shift / running_mean: bits of the specified function of the kernel's own mean / invstd (0 or inf)."""
    want = finalize_exact(mean, invstd, weight, bias, momentum, running_mean)
    return {k: (0.0 if same_bits(got[k], v) else float('inf')) for k, v in want.items()}


def apply_ratios(x, scale, shift, res, act, slope, y, bf16=False):
    yr, zr, mag = apply_ref(x, scale, shift, res, act, slope)
    return {'y': worst_ratio(_d(y) - yr, apply_gate(mag, yr, zr, act, res is not None, bf16))}


def partials_ratios(part, s1, s2):
    part = _d(part)
    k = (k_partials(part.shape[0]) + 1) * U64
    return {'s1': worst_ratio(_d(s1) - _colsum(part[:, 0]), k * _colsum(np.abs(part[:, 0]))),
            's2': worst_ratio(_d(s2) - _colsum(part[:, 1]), k * _colsum(np.abs(part[:, 1])))}


def bwd_ratios(x, dy, y_pos, mean, invstd, weight, scale, shift, act, slope, count, s1, s2, dx=None, dres=None, dweight=None,
               dbias=None, bf16=False):
    """The backward kernels alone: constants as handed to them; the mask of ReLU / LeakyReLU from the forward output (`y_pos`).
    s1, s2: the kernel's own sums (gated here; dx is then measured against the fp64 expression on those very sums)."""
    P, C = np.shape(x)
    out = {}
    zr = gz = None
    if act == ACT_SWISH:
        _, zr, mag = apply_ref(x, scale, shift, None, ACT_NONE, 0.0)
        gz = 2 * U32 * mag + DENORM
    g = masked_grad(dy, y_pos, act, slope, z=zr)
    # error of g itself: none for the mask family (an fp32 value, exact); swish: the derivative's gate and the fp32 product dy * d
    dg = None if act != ACT_SWISH else np.abs(_d(dy)) * swish_grad_gate(zr, gz) + U32 * np.abs(g)
    if dres is not None:
        gd = (0.0 if dg is None else dg) + (UBF * np.abs(g) if bf16 else 0.0)
        out['dres'] = (0.0 if same_bits(dres, bf16_rne(f32(g)) if bf16 else f32(g)) else float('inf')) if dg is None else worst_ratio(_d(dres) - g, gd + (UBF * gd if bf16 else 0))
    ref = bwd_sums_ref(x, g, mean, invstd)
    xh_abs = np.abs((_d(x) - _d(mean)) * _d(invstd))
    e1 = 0.0 if dg is None else _colsum(dg)
    e2 = 0.0 if dg is None else _colsum(dg * xh_abs)
    g1 = sum_gate(P, C, ref['a1'], bf16) + e1
    g2 = sum_gate(P, C, ref['a2'], bf16, extra=3) + e2
    out['s1'] = worst_ratio(_d(s1) - ref['s1'], g1); out['s2'] = worst_ratio(_d(s2) - ref['s2'], g2)
    if dbias is not None:                                # (float) of the fp64 sum: one more rounding
        out['dbias'] = worst_ratio(_d(dbias) - ref['s1'], g1 + U32 * (np.abs(ref['s1']) + g1) + DENORM)
        out['dweight'] = worst_ratio(_d(dweight) - ref['s2'], g2 + U32 * (np.abs(ref['s2']) + g2) + DENORM)
    if dx is not None:
        dr, mag = dx_ref(x, g, mean, invstd, weight, s1, s2, count)
        w_is = _d(invstd) * (1.0 if weight is None else _d(weight))
        out['dx'] = worst_ratio(_d(dx) - dr, dx_gate(dr, mag, bf16, dg, w_is))
    return out


def running_gates(ref, fin, K_rel, eps, var_mode, momentum, rm0, rv0):
    """Gates of the running estimates against finalize_ref, from zero / one initial values or any other:
    running_mean = fma(mom, (float) m, fl(fl(1 - mom) rm)): mom times the mean's gate, two roundings on the kept part, one on the result;
    running_var  = fma(mom, (float) unb, ...): mom times (dv n / (n - 1) + the roundings of the product, the division (fp64) and the cast)."""
    mg = moment_gates(ref, K_rel, eps, var_mode)
    n = ref['count']; mom = float(F32(momentum))
    unb = ref['var'] * n / (n - 1) if n > 1 else ref['var']
    dunb = mg['var'] * (n / (n - 1) if n > 1 else 1.0) + (U32 + 2 * U64) * unb
    keep = lambda r0: 2 * U32 * np.abs((1 - mom) * _d(r0))          # fl(fl(1 - mom) r0): two roundings of the kept part
    return dict(running_mean=mom * mg['mean'] + keep(rm0) + U32 * np.abs(fin['running_mean']) + DENORM,
                running_var=mom * dunb + keep(rv0) + U32 * np.abs(fin['running_var']) + DENORM)


def chain_ratios(x, weight, bias, res, act, slope, eps, var_mode, y, dy=None, dx=None, dres=None, dweight=None, dbias=None, bf16=False):
    """The assembled op (statistics -> finalize -> apply; reduce -> apply backward) against the fp64 chain.  The per-kernel gates,
    with the error of each stage's fp32 constants carried into the next by first-order propagation of the formulas:
      d_is, d_m      moment_gates (sum error of this geometry, one fp32 rounding)
      d_sc = |w| d_is + u32 |w is|                      sc = fl(w is)
      d_sh = |m| d_sc + |sc| d_m + u32 (|m sc| + |b|)   shift = fma(-m, sc, b)
      y    : apply_gate + |x| d_sc + d_sh               (through an activation of slope <= 1; 1.1 for swish)
      xhat : d_xh = |x - m| d_is + is d_m
      s1   : sum_gate(sum |g|);  s2: sum_gate(sum |g xhat|, 3 term roundings) + sum |g| d_xh      (swish: + the derivative's gate)
      dx   : dx_gate + |w| d_is (|g| + |m1| + |xhat m2|) + |w| is (d_s1 / n + |xhat| d_s2 / n + d_xh |m2|)
    The ReLU / LeakyReLU mask is the one of the forward output the op produced (y > 0), the kernels' contract."""
    P, C = np.shape(x)
    ref = stats_ref(x)
    n = ref['count']
    fin = finalize_ref(ref['mean'], ref['var'], n, weight, bias, eps, 0.1, var_mode)
    mg = moment_gates(ref, sum_rel(P, C, bf16), eps, var_mode)
    w = np.ones(C) if weight is None else _d(weight); b = np.zeros(C) if bias is None else _d(bias)
    m, is_, sc, sh = fin['mean'], fin['invstd'], fin['scale'], fin['shift']
    d_m, d_is = mg['mean'], mg['invstd']
    d_sc = np.abs(w) * d_is + U32 * np.abs(sc)
    d_sh = np.abs(m) * d_sc + np.abs(sc) * d_m + U32 * (np.abs(m * sc) + np.abs(b))
    yr, zr, mag = apply_ref(x, sc, sh, res, act, slope)
    carried = np.abs(_d(x)) * d_sc + d_sh
    lip = SWISH_LIP if act == ACT_SWISH else 1.0
    gz_fwd = (3 if res is not None else 2) * U32 * mag + DENORM + carried
    gy = apply_gate(mag, yr, zr, act, res is not None, False) + lip * carried
    out = {'y': worst_ratio(_d(y) - yr, gy + (UBF * (np.abs(yr) + gy) if bf16 else 0.0))}
    if dy is None:
        return out
    if act == ACT_SWISH:
        g = masked_grad(dy, None, act, slope, z=zr)
        dg = np.abs(_d(dy)) * swish_grad_gate(zr, gz_fwd) + U32 * np.abs(g)
    else:
        g = masked_grad(dy, _d(y) > 0, act, slope)
        dg = np.zeros_like(g)
    xc = _d(x) - m
    xh = xc * is_
    d_xh = np.abs(xc) * d_is + is_ * d_m
    sums = bwd_sums_ref(x, g, m, is_)
    d_s1 = sum_gate(P, C, sums['a1'], bf16) + _colsum(dg)
    d_s2 = sum_gate(P, C, sums['a2'], bf16, extra=3) + _colsum(np.abs(g) * d_xh + dg * (np.abs(xh) + d_xh))
    if dbias is not None:
        out['dbias'] = worst_ratio(_d(dbias) - sums['s1'], d_s1 + U32 * (np.abs(sums['s1']) + d_s1) + DENORM)
        out['dweight'] = worst_ratio(_d(dweight) - sums['s2'], d_s2 + U32 * (np.abs(sums['s2']) + d_s2) + DENORM)
    if dres is not None:
        out['dres'] = worst_ratio(_d(dres) - g, dg + (UBF * (np.abs(g) + dg) if bf16 else 0.0))
    if dx is not None:
        dr, dmag = dx_ref(x, g, m, is_, w, sums['s1'], sums['s2'], n)
        m2 = np.abs(sums['s2']) / n
        extra = np.abs(w) * d_is * dmag / np.maximum(np.abs(w) * is_, 1e-300) + np.abs(w) * is_ * (d_s1 / n + np.abs(xh) * d_s2 / n + d_xh * m2 + dg)
        gd = dx_gate(dr, dmag, bf16) + extra
        out['dx'] = worst_ratio(_d(dx) - dr, gd + ((UBF if bf16 else U32) * extra))
    return out
