"""CPU rehearsal of tests/dw_ref.py, the oracle of tests/test_dw_gpu.py, before a GPU sees it:

* the fp64 references agree with fp64 torch (F.conv2d with groups = C and autograd) to 1e-12 of the magnitude sum;
* the restated route equals ssg_dwconv2d_kernel_id of the built library at every case, op and dtype (and over a grid of
  arguments around every threshold), and the restated part / slice arithmetic equals the two workspace queries;
* the case tables reach every kernel id of every op in each dtype, KW 3/5/7/9 on the tiled routes, and every edge of the weight
  gradient's parts and of the channel sum's slices (check_coverage);
* an fp32 emulation of each tiled kernel's index arithmetic passes every gate of the GPU file at every case of the GPU file;
* each of the eleven planted defects fails its gate at a named case of the table.

Worst emulation error / gate over all cases of a family (pass: <= 1), as printed by this module with -s:

    forward          fp32 0.34 (stride 1), 0.28 (stride 2)                  bf16 0.995, 0.984
    input gradient   fp32 0.33 (stride 1), 0.22 / 0.18 (stride 2, PLODD 0 / 1)   bf16 0.996, 0.996 / 0.995
    weight gradient  fp32 0.983 (stride 1), 0.991 (stride 2)                bf16 0.19, 0.16
    channel sum      fp32 0.998 (a), 0.75 (a b)                             bf16 0.018, 0.020
    unary y, dx      swish 0.51, 0.40; sigmoid 0.50, 0.48; gaussian 0.91, 0.88

  (the fp32 weight gradient and channel sum and the bf16 stores are single roundings of an accurately known value: a half-ulp
  bound is met close to 1.  The emulation's expf is the rounding of the exact value: numpy's own fp32 exp errs by up to 2 ulp.)

The planted defects, each at its named cases (error / gate; inf = an output left unwritten):

     1 last column dropped when OW % 4 != 0 (w5_s1k3, ow3_s2k3_even / _odd)      inf
     2 left pad off by one (s1k3_same, s2k5_7x10_p1212, s1k5_same)              3.3e6 fwd, 2.6e5 bf16 S=2 fwd, 1.1e7 S=2 dgrad, 4.2e9 wgrad
     3 kernel not flipped, stride-1 input gradient (s1k5_same, s1k9_p0202)      2.0e6, 7.0e4 (bf16)
     4 PLODD inverted (s2k3 p0101 / p1111, s2k5 p1212 / p2222)                  2.0e10, 3.2e9, 1.4e5 (bf16), 2.5e5 (bf16)
     5 last x-quad of a part dropped (wg_ragged_s1, wg_ragged_s2, wg_onepart)   8.5e5, 2.1e3 (bf16), 6.5e5
     6 last part dropped (wg_ragged_s1, wg_capped)                              1.8e7, 43 (bf16, 1 part of 256)
     7 bias omitted (c8_s1k3, c60_s2k5)                                         1.4e6, 1.5e4 (bf16)
     8 bias added twice (c8_s1k3, c60_s2k5)                                     1.4e6, 1.5e4 (bf16)
     9 bf16 store truncates (c64_s1k3, c132_s2k5; forward and input gradient)   1.96, 1.95, 1.91, 1.98
    10 last slice of the channel sum dropped (2 x 4097 x 8)                     1.3e6 / 2.7e5 (fp32 a / a b), 2.3e4 / 1.8e4 (bf16)
    11 scale applied inside the slice loop (2 x 4097 x 8)                       1.6e7 / 2.2e6 (fp32), 3.0e5 / 1.5e5 (bf16)
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dw_ref as dr
from dw_ref import F64, OP_DGRAD, OP_FWD, OP_WGRAD

WORST = {}


def _note(key, v):
    WORST[key] = max(WORST.get(key, 0.0), v)
    return v


def _case(name, bf16=False):
    return next(c for c in dr.dw_cases(bf16) if c.name == name)


@pytest.fixture(scope='module')
def lib(pkg):
    return pkg._lib


# ----------------------------------------------------------------------------- the references against fp64 torch
@pytest.mark.parametrize('name', ['s2k5_7x10_p1212', 's2k3_8x9_p0101', 's1k9_p0202', 'rect3x5_s2', 'k4', 's3k3', 's4k5', 'w2_k9'])
def test_references_match_torch_fp64(name):
    c = _case(name)
    x, w, b, g = (np.asarray(a, dtype=F64) for a in dr.dw_data(c, False))
    pt, pb, pl, pr = c.pads
    xt = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 3, 1, 2))).requires_grad_(True)
    wt = torch.from_numpy(w[:, None]).requires_grad_(True)
    y = F.conv2d(F.pad(xt, (pl, pr, pt, pb)), wt, torch.from_numpy(b), stride=c.stride, groups=c.C)
    y.backward(torch.from_numpy(np.ascontiguousarray(g.transpose(0, 3, 1, 2))))
    ref, mag = dr.fwd_ref(x, w, b, c.stride, c.pads)
    assert ref.shape == g.shape
    assert dr.worst_ratio(y.detach().numpy().transpose(0, 2, 3, 1) - ref, 1e-12 * mag) <= 1
    dx, dmag = dr.dgrad_ref(g, w, c.stride, c.pads, c.H, c.W)
    assert dr.worst_ratio(xt.grad.numpy().transpose(0, 2, 3, 1) - dx, 1e-12 * dmag + 1e-300) <= 1
    dw, wmag = dr.wgrad_ref(x, g, c.KH, c.KW, c.stride, c.pads)
    assert dr.worst_ratio(wt.grad.numpy()[:, 0] - dw, 1e-12 * wmag + 1e-300) <= 1


def test_se_and_unary_references_match_torch_fp64():
    x, s = dr.se_data(3, 67, 60, False)
    xt, st = torch.from_numpy(x.astype(F64)), torch.from_numpy(s.astype(F64))
    assert np.allclose(dr.channel_scale_ref(x, s), (xt * st[:, None]).numpy(), rtol=1e-14, atol=0)
    ref, mag = dr.channel_sum_ref(x, x[::-1], 0.75)
    assert dr.worst_ratio((xt * torch.from_numpy(x[::-1].astype(F64))).sum(1).numpy() * 0.75 - ref, 1e-13 * mag) <= 1
    assert np.array_equal(dr.broadcast_ref(s, 0.25, 5), np.broadcast_to(0.25 * s.astype(F64)[:, None], (3, 5, 60)))
    z = torch.linspace(-30, 30, 241, dtype=torch.float64, requires_grad=True)
    for op, fn in ((dr.UNARY_SWISH, lambda t: t * torch.sigmoid(t)), (dr.UNARY_SIGMOID, torch.sigmoid), (dr.UNARY_GAUSSIAN, lambda t: torch.exp(-t * t))):
        y = fn(z)
        (d,) = torch.autograd.grad(y.sum(), z)
        yr, dref = dr.unary_ref(z.detach().numpy(), op)
        assert np.allclose(yr, y.detach().numpy(), rtol=1e-13, atol=1e-300) and np.allclose(dref, d.numpy(), rtol=1e-12, atol=1e-15)


# ----------------------------------------------------------------------------- route and geometry against the built library
def _lib_route(lib, op, stride, KH, KW, pl, ndh, C, aligned):
    return lib.call('ssg_dwconv2d_kernel_id', op, stride, KH, KW, pl, ndh, C, int(aligned))


def test_coverage():
    dr.check_coverage()
    dr.check_colsum_coverage()


def test_route_agrees_with_the_library_on_every_case(lib):
    n = 0
    for bf16 in (False, True):
        for c in dr.dw_cases(bf16):
            OH, OW = dr.out_hw(c.H, c.W, c.KH, c.KW, c.stride, c.pads)
            for op in (OP_FWD, OP_DGRAD, OP_WGRAD):
                ndh = c.N * (OH if op == OP_FWD else c.H)
                got = _lib_route(lib, op, c.stride, c.KH, c.KW, c.pads[2], ndh, c.C, dr.case_aligned(c, bf16))
                assert got == dr.case_route(c, op, bf16), (c.name, op, bf16, got)
                n += 1
    assert n == 3 * (2 * len(dr.DW_CASES) + len(dr.DW_CASES_BF16_UNALIGNED))


def test_route_agrees_with_the_library_around_every_threshold(lib):
    for op in (OP_FWD, OP_DGRAD, OP_WGRAD, 3, -1):
        for stride in (1, 2, 3, 4):
            for KH in (1, 3, 5, 7):
                for KW in range(1, 12):
                    for pl in (0, 1, 2, 3):
                        for ndh in (1, 65535, 65536):
                            for C, al in ((4, 1), (4, 0), (132, 1), (4194240, 1), (4194244, 1)):
                                assert _lib_route(lib, op, stride, KH, KW, pl, ndh, C, al) == dr.route(op, stride, KH, KW, pl, ndh, C, al), \
                                    (op, stride, KH, KW, pl, ndh, C, al)


def test_part_and_slice_arithmetic_agree_with_the_workspace_queries(lib):
    for c in dr.dw_cases(True):
        OH, OW = dr.out_hw(c.H, c.W, c.KH, c.KW, c.stride, c.pads)
        want = lib.call('ssg_dwconv2d_wgrad_workspace_bytes', c.N, OH, OW, c.C, c.KH, c.KW)
        assert want == dr.wgrad_workspace_bytes(c.N, OH, OW, c.C, c.KH, c.KW), c.name
        geo = dr.wgrad_geom(c.N, OH, OW, c.stride, c.KW)
        assert geo.parts * c.KH * c.KW * c.C * 8 <= want and geo.parts * geo.rows_per_part >= geo.units > (geo.parts - 1) * geo.rows_per_part
    for (N, S, C) in dr.COLSUM_CASES + [dr.COLSUM_LD[:3]] + [(n, s, c) for n in (1, 7, 64) for s in (1, 256, 1 << 20) for c in (4, 64, 68, 2688)]:
        assert lib.call('ssg_sample_channel_sum_workspace_bytes', N, S, C) == dr.colsum_workspace_bytes(N, S, C), (N, S, C)
        geo = dr.colsum_geom(N, S, C)
        assert geo.slices * geo.rows_per_slice >= S > (geo.slices - 1) * geo.rows_per_slice, 'no empty slice'


# ----------------------------------------------------------------------------- emulations pass every gate at every case
def conv_emul(c, op, bf16, x, w, b, g, **defects):
    """The tiled emulation the route names for (case, op), or None on a generic route."""
    rid = dr.case_route(c, op, bf16)
    pt, _, pl, _ = c.pads
    OH, OW = g.shape[1:3]
    if rid in (dr.FWD_S1, dr.FWD_S2):
        return dr.s1_emul(x, w, b, OH, OW, pt, pl, S=c.stride, bf16=bf16, **defects)
    if rid == dr.DGRAD_S1_FLIP:
        defects.setdefault('flip', True)
        return dr.s1_emul(g, w, None, c.H, c.W, c.KH - 1 - pt, c.KW - 1 - pl, S=1, bf16=bf16, **defects)
    if rid in (dr.DGRAD_S2_EVEN, dr.DGRAD_S2_ODD):
        return dr.dgrad_s2_emul(g, w, c.H, c.W, pt, pl, bf16=bf16, **defects)
    if rid in (dr.WGRAD_S1, dr.WGRAD_S2):
        return dr.wgrad_tiled_emul(x, g, c.KH, c.KW, c.stride, pt, pl, bf16=bf16, **defects)
    return None


def conv_ratio(c, op, bf16, got, x, w, b, g):
    taps = c.KH * c.KW
    if op == OP_FWD:
        ref, mag = dr.fwd_ref(x, w, b, c.stride, c.pads)
        return dr.conv_ratio(got, ref, mag, taps, bf16)
    if op == OP_DGRAD:
        ref, mag = dr.dgrad_ref(g, w, c.stride, c.pads, c.H, c.W)
        return dr.conv_ratio(got, ref, mag, taps, bf16)
    ref, mag = dr.wgrad_ref(x, g, c.KH, c.KW, c.stride, c.pads)
    return dr.wgrad_ratio(got, ref, mag, c, bf16)


@pytest.mark.parametrize('bf16', [False, True], ids=['f32', 'bf16'])
def test_emulations_pass_every_conv_gate(bf16):
    ran = set()
    for c in dr.dw_cases(bf16):
        data = dr.dw_data(c, bf16)
        for o in c.ops:
            got = conv_emul(c, dr.OPS[o], bf16, *data)
            if got is None:
                continue
            r = conv_ratio(c, dr.OPS[o], bf16, got, *data)
            rid = dr.case_route(c, dr.OPS[o], bf16)
            ran.add(rid)
            _note('%s id %d' % ('bf16' if bf16 else 'fp32', rid), r)
            assert r <= 1.0, (c.name, o, r)
    assert ran == set(dr.TILED_IDS)
    for k in sorted(WORST):
        print('RATIO emulation %-12s %.3g' % (k, WORST[k]))


@pytest.mark.parametrize('bf16', [False, True], ids=['f32', 'bf16'])
@pytest.mark.parametrize('case', dr.COLSUM_CASES + [dr.COLSUM_LD[:3]], ids=lambda c: '%dx%dx%d' % c)
def test_emulation_passes_the_channel_sum_gates(case, bf16):
    N, S, C = case
    a, b = dr.colsum_data(N, S, C, bf16)
    for bb, scale in ((None, 1.0 / S), (b, 0.75)):
        ref, mag = dr.channel_sum_ref(a, bb, scale)
        r = dr.colsum_ratio(dr.colsum_emul(a, bb, scale, bf16), ref, mag, N, S, C, bf16, bb is not None)
        print('RATIO emulation colsum %s %s %.3g' % ('bf16' if bf16 else 'fp32', 'a' if bb is None else 'ab', r))
        assert r <= 1.0


def test_emulation_passes_the_unary_gates():
    for (P, C, _, _) in dr.UNARY_CASES:
        z, g = dr.unary_data(P, C)
        assert z.size >= len(dr.Z_SWEEP)
        for op in (dr.UNARY_SWISH, dr.UNARY_SIGMOID, dr.UNARY_GAUSSIAN):
            y, dx = dr.unary_emul(z, op, g)
            yr, d = dr.unary_ref(z, op)
            gy, gd = dr.unary_gates(z, op, g)
            with np.errstate(all='ignore'):
                ry, rd = dr.unary_ratio(y, yr, gy), dr.unary_ratio(dx, g.astype(F64) * d, gd)
            print('RATIO emulation unary op %d y=%.3g dx=%.3g' % (op, ry, rd))
            assert ry <= 1.0 and rd <= 1.0, (P, C, op, ry, rd)


def test_one_rounding_gates_hold_for_correctly_rounded_products():
    for bf16 in (False, True):
        x, s = dr.se_data(3, 255, 132, bf16)
        y = dr._store((x.astype(F64) * s.astype(F64)[:, None]).astype(np.float32), bf16)
        assert dr.worst_ratio(y - dr.channel_scale_ref(x, s), dr.one_rounding_gate(dr.channel_scale_ref(x, s), bf16)) <= 1.0
        if bf16:
            bad = dr._store(f32_product(x, s), True, truncate=True)
            assert dr.worst_ratio(bad - dr.channel_scale_ref(x, s), dr.one_rounding_gate(dr.channel_scale_ref(x, s), True)) > 1.0


def f32_product(x, s):
    return (x.astype(F64) * s.astype(F64)[:, None]).astype(np.float32)


# ----------------------------------------------------------------------------- every planted defect fails a gate
def _defect(name, op, bf16=False, **defects):
    c = _case(name, bf16)
    data = dr.dw_data(c, bf16)
    good = conv_ratio(c, op, bf16, conv_emul(c, op, bf16, *data), *data)
    bad = conv_ratio(c, op, bf16, conv_emul(c, op, bf16, *data, **defects), *data)
    print('DEFECT %-16s %-16s %s: %.3g (clean %.3g)' % (name, sorted(defects)[0], 'bf16' if bf16 else 'fp32', bad, good))
    assert good <= 1.0 < bad, (name, defects, good, bad)


@pytest.mark.parametrize('name,op,bf16,defect', [
    ('w5_s1k3', OP_FWD, False, dict(drop_last_col=True)),
    ('w5_s1k3', OP_DGRAD, True, dict(drop_last_col=True)),
    ('ow3_s2k3_even', OP_FWD, False, dict(drop_last_col=True)),
    ('ow3_s2k3_odd', OP_DGRAD, False, dict(drop_last_col=True)),
    ('s1k3_same', OP_FWD, False, dict(pad_off=True)),
    ('s2k5_7x10_p1212', OP_FWD, True, dict(pad_off=True)),
    ('s2k5_7x10_p1212', OP_DGRAD, False, dict(pad_off=True)),
    ('s1k5_same', OP_WGRAD, False, dict(pad_off=True)),
    ('s1k5_same', OP_DGRAD, False, dict(flip=False)),
    ('s1k9_p0202', OP_DGRAD, True, dict(flip=False)),
    ('s2k3_7x10_p0101', OP_DGRAD, False, dict(plodd_inverted=True)),
    ('s2k3_8x9_p1111', OP_DGRAD, False, dict(plodd_inverted=True)),
    ('s2k5_8x9_p1212', OP_DGRAD, True, dict(plodd_inverted=True)),
    ('s2k5_7x10_p2222', OP_DGRAD, True, dict(plodd_inverted=True)),
    ('wg_ragged_s1', OP_WGRAD, False, dict(drop_last_quad=True)),
    ('wg_ragged_s2', OP_WGRAD, True, dict(drop_last_quad=True)),
    ('wg_onepart', OP_WGRAD, False, dict(drop_last_quad=True)),
    ('wg_ragged_s1', OP_WGRAD, False, dict(drop_last_part=True)),
    ('wg_capped', OP_WGRAD, True, dict(drop_last_part=True)),
    ('c8_s1k3', OP_FWD, False, dict(bias_omit=True)),
    ('c8_s1k3', OP_FWD, False, dict(bias_twice=True)),
    ('c60_s2k5', OP_FWD, True, dict(bias_omit=True)),
    ('c60_s2k5', OP_FWD, True, dict(bias_twice=True)),
    ('c64_s1k3', OP_FWD, True, dict(truncate=True)),
    ('c64_s1k3', OP_DGRAD, True, dict(truncate=True)),
    ('c132_s2k5', OP_FWD, True, dict(truncate=True)),
    ('c132_s2k5', OP_DGRAD, True, dict(truncate=True)),
], ids=lambda v: v if isinstance(v, str) else (sorted(v)[0] if isinstance(v, dict) else str(v)))
def test_planted_conv_defect_fails(name, op, bf16, defect):
    _defect(name, op, bf16, **defect)


@pytest.mark.parametrize('bf16', [False, True], ids=['f32', 'bf16'])
@pytest.mark.parametrize('defect', ['drop_last_slice', 'scale_per_slice'])
def test_planted_channel_sum_defect_fails(defect, bf16):
    N, S, C = 2, 4097, 8
    assert dr.colsum_geom(N, S, C).slices > 1
    a, b = dr.colsum_data(N, S, C, bf16)
    for bb, scale in ((None, 1.0 / S), (b, 0.75)):
        ref, mag = dr.channel_sum_ref(a, bb, scale)
        bad = dr.colsum_ratio(dr.colsum_emul(a, bb, scale, bf16, **{defect: True}), ref, mag, N, S, C, bf16, bb is not None)
        print('DEFECT colsum %s %s: %.3g' % (defect, 'bf16' if bf16 else 'fp32', bad))
        assert bad > 1.0
