"""CPU rehearsal of tests/bn_ref.py, the oracle of tests/test_bn_gpu.py, before a GPU sees it:

* the references agree with fp64 torch to 1e-12 (F.batch_norm with autograd for every activation, the biased / unbiased variance
  relation, the clamp(var, eps)^-1/2 of batchnorm.py);
* the restated red_geom and fold rule equal the library's host-only workspace queries at every case, and every case has the
  geometry fact it is listed for;
* an emulation of each kernel's arithmetic, in the kernel's grouping, passes every gate of the GPU file at every case of the GPU
  file (a gate the kernel's own arithmetic could exceed would be wrong);
* each of the eleven planted defects fails its gate at a named case (a gate that lets one through would be too wide).

Worst emulation error / gate over all cases of a family (pass: <= 1), as printed by this module with -s:

    statistics fp32             0.00 s1, 0.19 s2, 1.00 mean, 0.995 invstd, 0.90 channel sum     (K = rows/thread + PR + parts/32 + 32, + 1)
    statistics bf16             0.0003 s1, 0.04 s2, 0.39 mean, 0.70 invstd                      (per-thread part at 2^-24)
    partial rows                0.14 s1, 0.11 s2                                                (rows spread over 1e12)
    apply                       0.63 fp32, 0.45 fp32 swish, 0.996 bf16 and bf16 swish
    backward fp32               0.05 sums, 0.99 dweight, 1.00 dbias, 1.00 dx, dres exact;  swish: 0.51 sums, 0.64 dres, 0.93 dx
    backward bf16               0.47 sums, 0.44 dweight, 0.996 dx, dres exact;             swish: 0.43 sums, 0.99 dres, 0.996 dx
    scale / shift / running_mean / running_var: the emulation IS the specification (exact)

  (mean, dx, dbias and the bf16 stores are single roundings of an accurately known value: a half-ulp bound is met at 1.00.)

The planted defects, each at its named case (error / gate; inf = an exact comparison failed):

     1 s2 accumulated in fp32 (287 x 256)                8.2e6
     2 short last part dropped (2047 x 8)                2.7e13
     3 idle quad lane's LDS row added (1535 x 12)        8.5e13   (bf16, 1023 x 24: 2.1e6)
     4 fold rows beyond nz rpz dropped (257 rows)        3.3e12
     5 running_var without count / (count - 1)           inf      (off by up to 5.3e3 ulp at 319 x 260)
     6 var_mode 0 and 1 swapped (eps 1e-3)               9.4e5
     7 backward constants rounded to fp32 (767 x 40)     204
     8 mask by mul + add where the forward used fma      2052 (fp32) and 2024 (bf16) of 36 864 probe masks differ
     9 dres left unmasked (95 x 512)                     inf
    10 bf16 store truncates (1023 x 24)                  1.94
    11 pixel count from P instead of sums[2C]            1.6e8

bf16's unit roundoff is 2^-8 (8 significand bits), not 2^-9: test_bf16_unit_roundoff shows a correctly rounded store at 2^-8.
LeakyReLU's negative side carries one more fp32 rounding (the product with the slope) than ReLU's: apply_gate counts it there only.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bn_ref as br
from bn_ref import ACT_LRELU, ACT_NONE, ACT_RELU, ACT_SWISH, F32, F64, f32

SLOPE = 0.2
WORST = {}


def _note(family, ratios):
    for k, v in ratios.items():
        key = '%s %s' % (family, k)
        WORST[key] = max(WORST.get(key, 0.0), v)


def _report(family, ratios):
    print('RATIO %-28s %s' % (family, '  '.join('%s=%.3g' % kv for kv in sorted(ratios.items()))))


def _ok(ratios):
    return all(v <= 1.0 for v in ratios.values())


# ----------------------------------------------------------------------------- the references against fp64 torch
@pytest.mark.parametrize('act,res', [(ACT_NONE, False), (ACT_NONE, True), (ACT_RELU, False), (ACT_RELU, True), (ACT_LRELU, False),
                                     (ACT_LRELU, True), (ACT_SWISH, False)])        # swish with a residual is refused by the kernels
def test_references_match_torch_fp64(act, res):
    P, C, eps, mom = 37, 12, float(F32(1e-3)), float(F32(0.1))        # eps / momentum enter the kernels as fp32 values
    g = torch.Generator().manual_seed(5)
    t64 = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    nchw = lambda a: torch.from_numpy(np.ascontiguousarray(a.T)).view(1, C, P, 1).requires_grad_(True)      # [P, C] rows -> (1, C, P, 1)
    rows = lambda t: np.ascontiguousarray(t.detach().numpy().reshape(C, P).T)
    xn = (t64(P, C) * 2 + 1).numpy(); wn = t64(C).numpy(); bn = t64(C).numpy()
    rn = t64(P, C).numpy() if res else None
    dyn = t64(P, C).float().double().numpy()
    rm0 = t64(C).numpy(); rv0 = (torch.rand(C, generator=g, dtype=torch.float64) + 0.5).numpy()
    x = nchw(xn); w = torch.from_numpy(wn).requires_grad_(True); b = torch.from_numpy(bn).requires_grad_(True)
    r = nchw(rn) if res else None
    rm, rv = torch.from_numpy(rm0.copy()), torch.from_numpy(rv0.copy())
    z = F.batch_norm(x, rm, rv, w, b, True, mom, eps)
    if res:
        z = z + r
    y = {ACT_NONE: lambda t: t, ACT_RELU: F.relu, ACT_LRELU: lambda t: F.leaky_relu(t, float(F32(SLOPE))), ACT_SWISH: lambda t: t * torch.sigmoid(t)}[act](z)
    y.backward(nchw(dyn).detach())

    ref = br.stats_ref(xn)
    assert np.allclose(ref['var'], xn.var(axis=0), rtol=1e-12, atol=0) and np.allclose(ref['var'] * P / (P - 1), xn.var(axis=0, ddof=1), rtol=1e-12)
    fin = br.finalize_ref(ref['mean'], ref['var'], P, wn, bn, eps, mom, 0, rm0, rv0)
    yr, zr, mag = br.apply_ref(xn, fin['scale'], fin['shift'], rn, act, SLOPE)
    assert np.abs(yr - rows(y)).max() <= 1e-12 * np.abs(mag).max() and (mag >= np.abs(zr) * (1 - 1e-12)).all()
    assert np.abs(fin['running_mean'] - rm.numpy()).max() <= 1e-12 and np.abs(fin['running_var'] - rv.numpy()).max() <= 1e-12
    # backward, with the mask taken from the forward output as the kernels' contract says
    gg = br.masked_grad(dyn.astype(F32), yr > 0, act, SLOPE, z=zr)
    sums = br.bwd_sums_ref(xn, gg, fin['mean'], fin['invstd'])
    dxr, dmag = br.dx_ref(xn, gg, fin['mean'], fin['invstd'], wn, sums['s1'], sums['s2'], P)
    lr = 2e-8 if act == ACT_LRELU else 0                   # masked_grad forms dy * slope in fp32, as the kernel does: one fp32 rounding
    assert np.abs(dxr - rows(x.grad)).max() <= (1e-12 + 4 * lr) * dmag.max()
    assert np.abs(sums['s1'] - b.grad.numpy()).max() <= (1e-12 + lr) * sums['a1'].max()
    assert np.abs(sums['s2'] - w.grad.numpy()).max() <= (1e-12 + lr) * sums['a2'].max()
    if res:
        assert np.abs(gg - rows(r.grad)).max() <= (1e-12 + lr) * np.abs(gg).max()


def test_var_mode_1_is_the_clamp_of_batchnorm_py():
    var = np.array([0.0, 1e-7, 1e-5, 1e-4, 2.0])
    for eps in (1e-5, 1e-3):
        want = torch.from_numpy(var).clamp(eps).pow(-0.5).numpy()
        assert np.abs(br.invstd_of(var, eps, 1) - want).max() <= 1e-12 * want.max()
        assert np.abs(br.invstd_of(var, eps, 0) - (var + eps) ** -0.5).max() <= 1e-12 * want.max()
    fin = br.finalize_ref(np.zeros(1), np.array([3.0]), 1, None, None, 1e-5, 0.1, 0, np.zeros(1), np.ones(1))
    assert abs(fin['running_var'][0] - (0.1 * 3.0 + 0.9)) < 1e-7             # count == 1: the biased variance, no division by zero


def test_bf16_unit_roundoff():
    """bf16 keeps 8 significand bits: 1 + 2^-8 is midway between its neighbours 1 and 1 + 2^-7 and rounds (to even) to 1, an error
    of 2^-8 |value| / (1 + 2^-8).  A gate of 2^-9 |value| would fail a correct store."""
    v = F32(1 + 2.0 ** -8)
    got = torch.tensor([float(v)]).bfloat16().float().numpy()[0]
    assert br.bf16_rne(np.array([v]))[0] == got == F32(1)
    assert abs(float(got) - float(v)) > 2.0 ** -9 * float(v) and abs(float(got) - float(v)) <= br.UBF * float(v)
    a = f32(np.random.RandomState(0).standard_normal(4096) * 100)
    assert br.same_bits(br.bf16_rne(a), torch.from_numpy(a).bfloat16().float().numpy())
    assert (np.abs(br.bf16_trunc(a)) <= np.abs(a)).all()


def test_exact_helpers():
    rng = np.random.RandomState(1)
    a, b, c = (f32(rng.standard_normal(200)) for _ in range(3))
    got = np.array([br.fma32(a[i], b[i], c[i]) for i in range(200)], dtype=F32)
    assert np.abs(got.astype(F64) - (a.astype(F64) * b + c)).max() <= br.U32 * 8
    assert br.fma32(F32(1 + 2.0 ** -12), F32(1 + 2.0 ** -12), F32(-1)) == F32(2.0 ** -11 + 2.0 ** -24)     # a bit a rounded product loses
    assert br.fma64(1 + 2.0 ** -30, 1 + 2.0 ** -30, -1.0) == 2.0 ** -29 + 2.0 ** -60


# ----------------------------------------------------------------------------- geometry
def _all_pc():
    out = [(P, C) for P, C, _ in br.STAT_CASES_F32 + br.STAT_CASES_BF16] + br.CHANNEL_SUM_EXTRA + [(P, C) for P, C, _ in br.LDS_CASES + br.LDS_CASES_BF16]
    return out + [br.LD_CASE[:2], (27, 2048), (8 * 13 * 11, 40)]


def test_geometry_restatement_equals_the_library(pkg):
    call = pkg._lib.call
    for P, C in _all_pc():
        assert call('ssg_bn_workspace_bytes', P, C) == br.workspace_bytes(P, C), (P, C)
    for rows, C in br.PARTIAL_CASES:
        assert call('ssg_bn_stats_from_partials_workspace_bytes', rows, C) == br.partials_workspace_bytes(rows, C), (rows, C)


def test_every_case_has_the_fact_it_is_listed_for():
    for Q, cases in ((1, br.STAT_CASES_F32), (2, br.STAT_CASES_BF16)):
        for P, C, facts in cases:
            assert not br.check_facts(P, C, Q, facts), (P, C, facts, br.check_facts(P, C, Q, facts))
    tq = {br.red_geom(P, C).TQ for P, C, _ in br.STAT_CASES_F32}
    assert tq == {1, 2, 4, 8, 16, 32, 64}
    parts = {br.red_geom(P, C).parts for P, C, _ in br.STAT_CASES_F32}
    assert set(range(1, 32)) <= parts and {32, 64} <= parts and any(p > 32 and p % 32 for p in parts)
    f = lambda **kw: [c for c in br.STAT_CASES_F32 if all(c[2].get(k) == v for k, v in kw.items())]
    assert any(br.live_lanes_last_group(br.red_geom(P, C)) < br.red_geom(P, C).TQ for P, C, _ in br.STAT_CASES_F32 if C in (12, 40))
    assert f(P_lt_PR=True) and f(clamp=True) and len(f(clamp=True)) == 2 and f(shrinks=True) and f(live_last=1)
    assert any(C % 32 for _, C, _ in br.STAT_CASES_F32) and {256, 260, 384} <= {C for _, C, _ in br.STAT_CASES_F32}
    assert any(P == 1 for P, _, _ in br.STAT_CASES_F32)
    assert {C for _, C, _ in br.STAT_CASES_BF16} >= {8, 24, 512, 520}
    assert all(c in br.STAT_CASES_F32 for c in br.BWD_CASES_F32) and all(c in br.STAT_CASES_BF16 for c in br.BWD_CASES_BF16)
    # unclamped estimates never shrink (the derivation beside first_shrinking_p)
    assert br.first_shrinking_p(256) == 32 * br.MAX_PARTS + 1 and br.first_shrinking_p(512, 2) == 32 * br.MAX_PARTS + 1
    # the fold: 257 is the smallest, nz = 52 < 64 slices, the last one short
    assert br.fold_geom(256) == (False, 256, 1) and br.fold_geom(257) == (True, 5, 52) and 257 - 51 * 5 == 2
    assert br.fold_geom(4097) == (True, 65, 64) and br.fold_geom(300) == (True, 5, 60)
    # dynamic LDS of bn_bwd_apply: 5 C doubles
    for P, C, optin in br.LDS_CASES + br.LDS_CASES_BF16:
        assert (5 * C * 8 > 48 * 1024) == optin and P <= 32 and C % 4 == 0
    assert all(C % 8 == 0 for _, C, _ in br.LDS_CASES_BF16) and 5 * 1224 * 8 <= 48 * 1024
    assert 5 * 1228 * 8 <= 48 * 1024 < 5 * 1232 * 8 and 5 * 4096 * 8 == 160 * 1024


# ----------------------------------------------------------------------------- every emulation through every gate
def _stats_rehearsal(P, C, bf16, seed=3, eps=1e-5, var_mode=0, **defects):
    x = br.stats_data(P, C, seed, bf16)
    ref = br.stats_ref(x)
    s1, s2 = br.stats_emul(x, bf16, **defects)
    r = br.stats_ratios(x, s1, s2, bf16, ref)
    w, b = br.affine_data(C, seed + 1)
    fin = br.finalize_emul(s1, s2, P, w, b, eps, 0.1, var_mode, np.zeros(C, F32), np.ones(C, F32))
    r.update(br.moment_ratios(ref, fin['mean'], fin['invstd'], br.sum_rel(P, C, bf16), eps, var_mode))
    return r, x, fin, (w, b)


@pytest.mark.parametrize('case', br.STAT_CASES_F32 + br.CHANNEL_SUM_EXTRA, ids=lambda c: '%dx%d' % c[:2])
def test_stats_emulation_f32(case):
    P, C = case[:2]
    if C % 4:                                            # channel_sum only
        x = br.stats_data(P, C, 3)
        s1, _ = br.col_reduce_emul(x.astype(F64), np.zeros_like(x, dtype=F64))
        ref = br.stats_ref(x)
        g = br.sum_gate(P, C, ref['a1'])
        r = {'fsum': br.worst_ratio(s1.astype(F32).astype(F64) - ref['s1'], g + br.U32 * (np.abs(ref['s1']) + g))}
    else:
        r, _, _, _ = _stats_rehearsal(P, C, False, eps=1e-5 if P % 2 else 1e-3, var_mode=(P // 2) % 2)
    _note('stats f32', r)
    assert _ok(r), r


@pytest.mark.parametrize('case', br.STAT_CASES_BF16, ids=lambda c: '%dx%d' % c[:2])
def test_stats_emulation_bf16(case):
    P, C = case[:2]
    r, _, _, _ = _stats_rehearsal(P, C, True, var_mode=P % 2)
    _note('stats bf16', r)
    assert _ok(r), r


@pytest.mark.parametrize('rows,C', br.PARTIAL_CASES)
def test_partials_emulation(rows, C):
    part = br.partial_rows(rows, C, rows)
    r = br.partials_ratios(part, *br.partials_emul(part))
    _note('partial rows', r)
    assert _ok(r), r


APPLY_F32 = [(1, 4), (3, 4), (767, 40), (319, 260), (32773, 256)]
APPLY_BF16 = [(1, 8), (1023, 24), (159, 520), (32773, 512)]
ACT_RES = [(ACT_NONE, False), (ACT_NONE, True), (ACT_RELU, False), (ACT_RELU, True), (ACT_LRELU, False), (ACT_LRELU, True), (ACT_SWISH, False)]


def _apply_inputs(P, C, bf16, res, seed=7):
    x = br.stats_data(P, C, seed, bf16)
    _, _, _, _, scale, shift = br.bwd_consts(x, C, seed + 1)
    r = br.grad_data(P, C, seed + 2, bf16) if res else None
    return x, scale, shift, r


@pytest.mark.parametrize('bf16,P,C', [(False,) + s for s in APPLY_F32] + [(True,) + s for s in APPLY_BF16])
def test_apply_emulation(bf16, P, C):
    for act, res in (ACT_RES if P * C < br.BIG else [(ACT_LRELU, True), (ACT_SWISH, False)]):
        x, scale, shift, r = _apply_inputs(P, C, bf16, res)
        _, zr, _ = br.apply_ref(x, scale, shift, r, act, SLOPE)
        assert act != ACT_SWISH or np.abs(zr).max() <= 10
        y = br.apply_emul(x, scale, shift, r, act, SLOPE, bf16)
        rr = br.apply_ratios(x, scale, shift, r, act, SLOPE, y, bf16)
        _note('apply %s%s' % ('bf16' if bf16 else 'f32', ' swish' if act == ACT_SWISH else ''), rr)
        assert _ok(rr), (act, res, rr)


def _bwd_rehearsal(P, C, bf16, act, with_y, seed=11, weight=True, **defects):
    x = br.stats_data(P, C, seed, bf16)
    dy = br.grad_data(P, C, seed + 1, bf16)
    w, b, mean, invstd, scale, shift = br.bwd_consts(x, C, seed + 2, affine=weight)
    y = br.apply_emul(x, scale, shift, None, act, SLOPE, bf16)
    mask_kw = {k: defects.pop(k) for k in ('mask_muladd',) if k in defects}
    red_kw = {k: defects.pop(k) for k in ('drop_short_last', 'idle_lane') if k in defects}
    g = br.masked_grad_emul(x, y if with_y else None, dy, scale, shift, act, SLOPE, **mask_kw)
    s1, s2 = br.bwd_reduce_emul(x, g, mean, invstd, bf16, **red_kw)
    dx = br.bwd_apply_emul(x, g, mean, invstd, w, s1, s2, P, bf16, **defects)
    dres = br.bf16_rne(g) if bf16 else g
    return br.bwd_ratios(x, dy, y > 0, mean, invstd, w, scale, shift, act, SLOPE, P, s1, s2, dx=dx, dres=dres,
                         dweight=s2.astype(F32), dbias=s1.astype(F32), bf16=bf16)


@pytest.mark.parametrize('case', br.BWD_CASES_F32 + [c + (None,) for c in br.LDS_CASES], ids=lambda c: '%dx%d' % c[:2])
def test_backward_emulation_f32(case):
    P, C = case[:2]
    plans = ((ACT_NONE, False), (ACT_RELU, True), (ACT_LRELU, False), (ACT_SWISH, False))
    for act, with_y in (plans[1::2] if P * C >= br.BIG else plans):               # as the GPU file: two plans at the 34-MB shapes
        r = _bwd_rehearsal(P, C, False, act, with_y, weight=(act != ACT_RELU or P * C >= br.BIG))
        _note('backward f32%s' % (' swish' if act == ACT_SWISH else ''), r)
        assert _ok(r), (act, r)


@pytest.mark.parametrize('case', br.BWD_CASES_BF16 + [c + (None,) for c in br.LDS_CASES_BF16], ids=lambda c: '%dx%d' % c[:2])
def test_backward_emulation_bf16(case):
    P, C = case[:2]
    for act, with_y in ((ACT_NONE, False), (ACT_RELU, True), (ACT_SWISH, False))[1 if P * C >= br.BIG else 0:]:
        r = _bwd_rehearsal(P, C, True, act, with_y)
        _note('backward bf16%s' % (' swish' if act == ACT_SWISH else ''), r)
        assert _ok(r), (act, r)


@pytest.mark.parametrize('bf16', [False, True])
def test_mask_probe_rehearsal(bf16):
    """The exact mask test of the GPU file on the emulation: every pre-activation within rounding of 0; the recomputed mask (one fma,
    as the forward) equals y > 0 everywhere, and defect 8 (mul + add) does not."""
    C, P = 2048, 18
    x, scale, shift = br.mask_probe(C, P, 21, bf16)
    z = br.preact_emul(x, scale, shift)
    assert np.abs(z).max() <= 8 * (2.0 ** -7 if bf16 else 2.0 ** -23) * 16 * 4 and (z > 0).any() and (z <= 0).any()
    y = br.apply_emul(x, scale, shift, None, ACT_LRELU, SLOPE, bf16)
    assert ((y > 0) == (z > 0)).all()                    # no tiny positive pre-activation that the bf16 store flushes
    dy = np.ones((P, C), F32)
    want = np.where(y > 0, F32(1), F32(SLOPE))
    good = br.masked_grad_emul(x, None, dy, scale, shift, ACT_LRELU, SLOPE)
    bad = br.masked_grad_emul(x, None, dy, scale, shift, ACT_LRELU, SLOPE, mask_muladd=True)
    assert br.same_bits(good, want) and br.same_bits(br.masked_grad_emul(x, y, dy, scale, shift, ACT_LRELU, SLOPE), want)
    n_bad = int((bad != want).sum())
    print('DEFECT 8 mask mul+add (%s): %d of %d masks differ' % ('bf16' if bf16 else 'f32', n_bad, P * C))
    assert n_bad > 0
    relu = br.masked_grad_emul(x, None, dy, scale, shift, ACT_RELU, 0.0)
    assert np.array_equal(relu.sum(axis=0), (y > 0).sum(axis=0).astype(F32))


@pytest.mark.parametrize('z0', [20.0, 90.0, 104.0])
def test_swish_limits_rehearsal(z0):
    for z in (z0, -z0):
        y = br.apply_emul(np.array([[z]], F32), np.ones(1, F32), np.zeros(1, F32), None, ACT_SWISH, 0.0)[0, 0]
        d = br.swish_grad_emul(np.array([z], F32))[0]
        assert br.swish_limit_ok(z, y, d), (z, y, d)


# ----------------------------------------------------------------------------- the planted defects
def test_planted_defects_fail():
    out = {}
    r, _, _, _ = _stats_rehearsal(287, 256, False, s2_f32=True)
    out['1 s2 in fp32 (287 x 256)'] = max(r['s2'], r['invstd'])
    r, _, _, _ = _stats_rehearsal(2047, 8, False, drop_short_last=True)
    out['2 short last part dropped (2047 x 8)'] = max(r['s1'], r['s2'])
    r, _, _, _ = _stats_rehearsal(1535, 12, False, idle_lane=True)
    out['3 idle lane row added (1535 x 12)'] = max(r['s1'], r['s2'])
    r, _, _, _ = _stats_rehearsal(1023, 24, True, idle_lane=True)
    out['3 idle lane row added, bf16 (1023 x 24)'] = max(r['s1'], r['s2'])
    part = br.partial_rows(257, 40, 257)
    out['4 fold tail dropped (257 rows)'] = max(br.partials_ratios(part, *br.partials_emul(part, drop_tail=True)).values())
    # 5, 6, 11: finalize
    P, C = 319, 260
    x = br.stats_data(P, C, 3)
    ref = br.stats_ref(x)
    s1, s2 = br.stats_emul(x)
    w, b = br.affine_data(C, 4)
    rv0 = np.ones(C, F32)
    good = br.finalize_emul(s1, s2, P, w, b, 1e-3, 0.1, 1, np.zeros(C, F32), rv0)
    bad = br.finalize_emul(s1, s2, P, w, b, 1e-3, 0.1, 1, np.zeros(C, F32), rv0, no_unbias=True)
    assert br.same_bits(good['running_var'], br.running_var_exact(s1, s2, P, 0.1, rv0)[0])
    out['5 running_var biased (319 x 260)'] = float('inf') if not br.same_bits(bad['running_var'], good['running_var']) else 0.0
    print('DEFECT 5: running_var off by up to %.3g ulp' % (np.abs(bad['running_var'] - good['running_var']) / np.spacing(good['running_var'])).max())
    bad = br.finalize_emul(s1, s2, P, w, b, 1e-3, 0.1, 1, swap_var_mode=True)
    out['6 var_mode swapped (eps 1e-3)'] = br.moment_ratios(ref, bad['mean'], bad['invstd'], br.sum_rel(P, C), 1e-3, 1)['invstd']
    bad = br.finalize_emul(s1, s2, P - 3 * 29, w, b, 1e-3, 0.1, 1)          # a 5-image shard's own count where sums[2C] = 8 images' should be read
    out['11 count from P (shard of 8 x 29 + ...)'] = max(br.moment_ratios(ref, bad['mean'], bad['invstd'], br.sum_rel(P, C), 1e-3, 1).values())
    out['7 backward constants in fp32 (767 x 40)'] = _bwd_rehearsal(767, 40, False, ACT_NONE, False, consts_f32=True)['dx']
    # 9: dres left unmasked
    x = br.stats_data(95, 512, 11); dy = br.grad_data(95, 512, 12)
    w, b, mean, invstd, scale, shift = br.bwd_consts(x, 512, 13)
    y = br.apply_emul(x, scale, shift, None, ACT_RELU, 0.0)
    g = br.masked_grad_emul(x, y, dy, scale, shift, ACT_RELU, 0.0)
    s1, s2 = br.bwd_reduce_emul(x, g, mean, invstd)
    out['9 dres unmasked (95 x 512)'] = br.bwd_ratios(x, dy, y > 0, mean, invstd, w, scale, shift, ACT_RELU, 0.0, 95, s1, s2, dres=dy)['dres']
    # 10: truncating bf16 store
    x, scale, shift, _ = _apply_inputs(1023, 24, True, False)
    y = br.apply_emul(x, scale, shift, None, ACT_NONE, 0.0, True, truncate=True)
    out['10 bf16 store truncates (1023 x 24)'] = br.apply_ratios(x, scale, shift, None, ACT_NONE, 0.0, y, True)['y']
    for k in sorted(out, key=lambda s: int(s.split()[0])):
        print('DEFECT %-46s %.3g' % (k, out[k]))
    assert all(v > 1.0 for v in out.values()), out


def test_zz_report():
    """Prints the worst ratio per family of this run (the figures of the module docstring)."""
    fams = sorted({k.rsplit(' ', 1)[0] for k in WORST})
    for fam in fams:
        _report(fam, {k.rsplit(' ', 1)[1]: v for k, v in WORST.items() if k.rsplit(' ', 1)[0] == fam})
    assert all(v <= 1.0 for v in WORST.values())
