"""CPU rehearsal of tests/test_frozen_bn_gpu.py: a numpy emulation of ssg_bn_frozen_bwd_f32 and ssg_bn_fold_bwd_f32 (tests/frozen_bn_ref.py)
goes through every gate of the GPU file at its very cases and passes; each planted defect fails:

    mask taken from x where y was saved | dx without scale | second sum over raw x instead of xhat | fold backward without the
    -mean sum_g term | dw not scaled by s

and the fold identity itself is checked against stock autograd in fp64."""
import numpy as np
import pytest
import torch

import bn_ref as br
import frozen_bn_ref as fr
from bn_ref import ACT_LRELU, ACT_NONE, ACT_RELU, ACT_SWISH, F32, F64, f32

GEOMS = [c[:2] for c in br.STAT_CASES_F32] + [br.LD_CASE[:2]]


def _ok(r):
    return all(v <= 1.0 for v in r.values())


def _case(P, C, seed):
    mean, invstd, w, b, scale, shift = fr.frozen_consts(C, seed)
    x = fr.frozen_x(P, C, mean, invstd, seed + 1)
    dy = br.grad_data(P, C, seed + 2)
    res = f32(np.random.RandomState(seed + 3).standard_normal((P, C)) * 2.0)
    return x, dy, res, mean, invstd, scale, shift


@pytest.mark.parametrize('P,C', GEOMS, ids=lambda v: str(v))
def test_emulation_passes_every_gate(P, C):
    """The GPU file's matrix at every geometry, the two of 2^22 elements and more included: per activation, mask recomputed (y NULL) and
    mask from a forward with residual (y given), and the x = mean = scale = NULL form.  (dres = NULL, a second run and y for the
    activations that ignore it change no arithmetic: the GPU file compares those bit for bit on the device.)"""
    x, dy, res, mean, invstd, scale, shift = _case(P, C, 100 + C)
    for act in fr.ACTS:
        slope = fr.slope_of(act)
        y_plain = br.apply_emul(x, scale, shift, None, act, slope)
        plans = [(None, y_plain > 0)]
        if act in (ACT_RELU, ACT_LRELU):
            y_res = br.apply_emul(x, scale, shift, res, act, slope)
            plans.append((y_res, y_res > 0))
        for y, pos in plans:
            dx, dres, s1, s2 = fr.frozen_bwd_emul(x, y, dy, mean, invstd, scale, shift, act, slope)
            r = fr.frozen_ratios(x, pos, dy, mean, invstd, scale, shift, act, slope, dx=dx, dres=dres, s1=s1, s2=s2)
            assert _ok(r), (act, y is not None, r)
        if act != ACT_SWISH:                             # activation backward + bias gradient: x = mean = scale = NULL
            y = plans[-1][0] if act != ACT_NONE else None
            gx, gres, g1, g2 = fr.frozen_bwd_emul(None, y, dy, None, None, None, None, act, slope)
            assert gx.tobytes() == dres.tobytes() and gres.tobytes() == dres.tobytes() and g1.tobytes() == s1.tobytes() and not g2.any()
            r = fr.frozen_ratios(None, plans[-1][1], dy, None, None, None, None, act, slope, dx=gx, dres=gres, s2=g2)
            assert _ok(r) and r['dx'] == 0.0 and r['s2'] == 0.0, r


def _assembled_case(act, with_res, **defects):
    """ops.batch_norm_act in eval mode, emulated, against fp64 autograd through F.batch_norm(training=False) at the variance whose
    rsqrt(var + eps) is the layer's fp32 invstd -- what tests/test_frozen_bn_gpu.py::test_batch_norm_act_eval_backward does on the GPU."""
    n, C, h, w = fr.ASSEMBLED[0]
    P = n * h * w
    eps = 1e-5
    mean, invstd, wt, bs, scale, shift = fr.frozen_consts(C, 60 + C)
    x = fr.frozen_x(P, C, mean, invstd, 71); dy = br.grad_data(P, C, 72)
    res = f32(np.random.RandomState(73).standard_normal((P, C)) * 2) if with_res else None
    slope = fr.slope_of(act)
    y = br.apply_emul(x, scale, shift, res, act, slope)
    keep_y = with_res and act in (ACT_RELU, ACT_LRELU)
    dx, dres, s1, s2 = fr.frozen_bwd_emul(x, y if keep_y else None, dy, mean, invstd, scale, shift, act, slope, **defects)
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=F64).reshape(n, h, w, -1)).permute(0, 3, 1, 2)
    rows = lambda g: np.ascontiguousarray(g.permute(0, 2, 3, 1).reshape(-1, C).numpy())
    x64 = t(x).clone().requires_grad_(True); r64 = t(res).clone().requires_grad_(True) if with_res else None
    w64 = torch.from_numpy(wt).double().requires_grad_(True); b64 = torch.from_numpy(bs).double().requires_grad_(True)
    var64 = 1.0 / torch.from_numpy(invstd).double() ** 2 - eps
    z = torch.nn.functional.batch_norm(x64, torch.from_numpy(mean).double(), var64, w64, b64, False, 0.0, eps)
    if with_res:
        z = z + r64
    pos = t(y) > 0
    out = z * torch.sigmoid(z) if act == ACT_SWISH else z if act == ACT_NONE else torch.where(pos, z, z * (0.0 if act == ACT_RELU else float(F32(slope))))
    out.backward(t(dy))
    ref = dict(dx=rows(x64.grad), dweight=w64.grad.numpy(), dbias=b64.grad.numpy())
    got = dict(dx=dx, dweight=s2.astype(F32), dbias=s1.astype(F32))
    if with_res:
        ref['dres'] = rows(r64.grad); got['dres'] = dres if act != ACT_NONE else dy
    return fr.assembled_ratios(x, y > 0, dy, mean, invstd, scale, shift, act, slope, ref, got)


@pytest.mark.parametrize('act,with_res', [(a, r) for a in fr.ACTS for r in (False, True) if not (a == ACT_SWISH and r)])
def test_assembled_gate_on_the_emulation(act, with_res):
    r = _assembled_case(act, with_res)
    assert _ok(r), r


def test_assembled_gate_fails_planted_defects():
    assert _assembled_case(ACT_LRELU, True, dx_no_scale=True)['dx'] > 1.0
    assert _assembled_case(ACT_RELU, True, mask_from_x=True)['dres'] > 1.0
    assert _assembled_case(ACT_NONE, False, s2_raw_x=True)['dweight'] > 1.0


def test_mask_probe_recomputed_mask_is_exact():
    C, P = 2048, 18
    x, scale, shift = br.mask_probe(C, P, 21)
    dy = np.ones((P, C), F32)
    for act in (ACT_RELU, ACT_LRELU):
        y = br.apply_emul(x, scale, shift, None, act, fr.slope_of(act))
        assert (y > 0).any() and (~(y > 0)).any()
        for yy in (None, y):
            _, dres, _, _ = fr.frozen_bwd_emul(x, yy, dy, None, None, scale, shift, act, fr.slope_of(act), reduce=False)
            assert _ok(fr.frozen_ratios(x, y > 0, dy, None, None, scale, shift, act, fr.slope_of(act), dres=dres))
        # a recomputed pre-activation that is mul + add instead of the forward's fma flips masks here: the gate sees it
        g = br.masked_grad_emul(x, None, dy, scale, shift, act, fr.slope_of(act), mask_muladd=True)
        assert not _ok(fr.frozen_ratios(x, y > 0, dy, None, None, scale, shift, act, fr.slope_of(act), dres=g))


@pytest.mark.parametrize('defect,key', [('mask_from_x', 'dres'), ('dx_no_scale', 'dx'), ('s2_raw_x', 's2')])
def test_planted_defects_fail(defect, key):
    P, C = br.LD_CASE[:2]
    x, dy, res, mean, invstd, scale, shift = _case(P, C, 7)
    y = br.apply_emul(x, scale, shift, res, ACT_RELU, 0.0)
    good = fr.frozen_bwd_emul(x, y, dy, mean, invstd, scale, shift, ACT_RELU, 0.0)
    bad = fr.frozen_bwd_emul(x, y, dy, mean, invstd, scale, shift, ACT_RELU, 0.0, **{defect: True})
    names = ('dx', 'dres', 's1', 's2')
    rg = fr.frozen_ratios(x, y > 0, dy, mean, invstd, scale, shift, ACT_RELU, 0.0, **dict(zip(names, good)))
    rb = fr.frozen_ratios(x, y > 0, dy, mean, invstd, scale, shift, ACT_RELU, 0.0, **dict(zip(names, bad)))
    assert _ok(rg), rg
    assert rb[key] > 1.0, rb


@pytest.mark.parametrize('Cout,K', fr.FOLD_CASES)
def test_fold_emulation_and_defects(Cout, K):
    data = fr.fold_data(Cout, K, 50 + Cout)
    dw, dg, db = fr.fold_bwd_emul(*data)
    r = fr.fold_ratios(*data, dw=dw, dgamma=dg, dbeta=db)
    assert _ok(r) and r['dw'] == 0.0, r
    dw, dg, db = fr.fold_bwd_emul(*data, no_mean_term=True)
    assert fr.fold_ratios(*data, dgamma=dg, dbeta=db)['dgamma'] > 1.0
    dw, _, _ = fr.fold_bwd_emul(*data, dw_unscaled=True)
    assert fr.fold_ratios(*data, dw=dw)['dw'] > 1.0


def test_fold_identity_against_autograd_fp64():
    """dW = dWf s, dgamma = (sum_k dWf W - mean sum_g) invstd, dbeta = sum_g are the gradients stock autograd gives for
    conv(x, W gamma invstd) + beta - mean gamma invstd with constant statistics."""
    g = torch.Generator().manual_seed(3)
    o, i = 5, 4
    W = torch.randn(o, i, 3, 3, generator=g, dtype=torch.float64, requires_grad=True)
    gamma = torch.randn(o, generator=g, dtype=torch.float64, requires_grad=True)
    beta = torch.randn(o, generator=g, dtype=torch.float64, requires_grad=True)
    mean = torch.randn(o, generator=g, dtype=torch.float64) * 10
    invstd = torch.rand(o, generator=g, dtype=torch.float64) + 0.5
    x = torch.randn(2, i, 6, 5, generator=g, dtype=torch.float64)
    up = torch.randn(2, o, 6, 5, generator=g, dtype=torch.float64)
    s = gamma * invstd
    y = torch.nn.functional.conv2d(x, W * s.view(-1, 1, 1, 1), beta - mean * s, padding=1)
    dW, dgm, dbt = torch.autograd.grad(y, (W, gamma, beta), up)
    dWf = torch.nn.functional.grad.conv2d_weight(x, W.shape, up, padding=1)
    sg = up.sum(dim=(0, 2, 3))
    t = (dWf * W.detach()).sum(dim=(1, 2, 3))
    for got, want in ((dWf * s.detach().view(-1, 1, 1, 1), dW), ((t - mean * sg) * invstd, dgm), (sg, dbt)):
        assert (got - want).abs().max().item() <= 1e-13 * want.abs().max().item()
