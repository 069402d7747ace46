"""CPU rehearsal of tests/conv_ref.py, the oracle of tests/test_conv_gpu.py, before a GPU sees it:

* at every case the descriptor is built with dummy 16-byte-aligned addresses (nothing launched or dereferenced) and the built library
  names the case's literal kernel id, pack format (ssg_conv2d_split_bn), split-K workspace, statistics rows and LDS-DMA body, and
  says yes to the fused input transform / backward statistics where the case uses them; check_coverage passes; the integer class
  stays below 2^24 at every case;
* conv_ref agrees with fp64 torch: F.conv2d (with bias, residual, activation, stride, concat, pad channels) and
  torch.nn.grad.conv2d_input (stride 1, a row slice, every parity class and the merged launch at odd sizes);
* the restated packs are self-consistent (the split planes add up to the fp32 pack, every slot is written once);
* the clean float32 emulation passes every gate -- classes (a), (b), (c), the 1 % activation-tie cap, the statistics gates;
* each planted defect (emul's seventeen switches; the two unwritten-tile switches share a row below) fails the gate meant for it.

Defect -> gate (the case it is shown on; what the gate reports, as printed by this module with -s):

     1 tap 0 one column off (halo32_c32_136)                       class (a): 18918 of 40392 elements differ
     2 ky / kx transposed (x3_41_c32_64)                           class (a): 13158 of 19008 (the six off-diagonal taps)
     3 dgrad taps not mirrored (halo33_dgrad)                      class (a): 30332 of 30420
     4 in2's channels one chunk further (k32_61_w17_cat, x3_41_cat_192)   class (a): 29376 of 29376, 32640 of 32640
     5 last K-step dropped (k32_60_w33)                            class (a): 45518 of 92928 (every element the ReLU passes)
     6 last slab dropped (splitk32_c176_40)                        class (a): 6087 of 11880 (likewise)
     7 last column / row of tiles not written (k32_60_w33)         NaN left at 3 % / 27 % of the grid's pixels
     8 a pad lane written (reg0_c24_134)                           the pad-lane check (class (a) itself passes)
     9 input transform applied to padding pixels (k32_60_aff_relu) class (a): 11160 of 92928 (the border pixels)
    10 leaky slope on the wrong sign (reg1_c24_40)                 class (a): 25821 of 25840
    11 mask of bwd_x from the gradient (k32_60_bwd_relu)           class (a): 46253 of 92928
    12 parity classes at each other's phase (parity_c16_64)        class (a): 46974 of 94080, and NaN left at 4 % of the pixels (odd sizes: the
       ... and one class launch at the wrong phase (reg1_s2_cls)   grids differ); the single class: every pixel of its phase NaN, others written
    13 third bf16 term of x dropped (k32_60_w33)                   class (b) only: `wpow2` no longer exact, `full` at 2.3 x the gate;
                                                                   classes (a) and (c) pass (hard gate 0.074)
    14 x2 w2 product dropped (k32_60_w33)                          class (b) `full` only, 8.4 x the gate; (a), (b) with a power of two and (c)
                                                                   pass (0.072)
    15 stride-2 taps read at unit stride (dma20_s2_c32_136)        class (a): 11069 of 21760
    16 residual added before the statistics (halo32_bn + res)      the totals gates of the rows: S1 at 6.7e3 x, S2 at 3.6e3 x

The clean emulation at the thirty-two `stat` cases: class (a) exact, class (b) exact with a power-of-two operand and 0.09 .. 0.46
(split routes) / 0.20 .. 0.46 (fp32 routes, where the epilogue's roundings are part of the gate) of the one-product gate at full
mantissas, class (c) at most 0.14 of the hard gate with at most 0.15 % activation ties.  At the twenty-four small cases with
statistics rows the totals lie within 0.027 (S1) / 0.015 (S2) of their gates, and one pixel missing from a row puts S1 at 15 .. 2900 x
its gate.  With one product of 288 missing, 98 % of the elements of k32_60_w33 that its ReLU passes exceed the hard gate.
The figures are printed by the tests (DEFECT / EMUL lines)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_ref as cr
from conv_ref import ACT_LRELU, ACT_NONE, F32, F64

A = 1 << 32                                 # dummy addresses: 16-byte aligned, distinct, never dereferenced
ADDR = {n: A * (i + 1) for i, n in enumerate('in1 in2 w bias res out scale shift bx bscale bshift bmean'.split())}


@pytest.fixture(scope='module')
def lib(pkg):
    yield pkg._lib
    pkg._lib.call('ssg_conv_set_k32_mode', 1)


def _ids(c):
    return c.name


# ----------------------------------------------------------------------------- literals and coverage
@pytest.mark.parametrize('c', cr.CASES, ids=_ids)
def test_library_names_the_literals(lib, c):
    D = cr.fill_desc(lib.ConvDesc(), c, ADDR)
    p = cr.plan_queries(lib, c, D, lambda fmt: 20 * A, lambda rows: 21 * A, lambda nbytes: 22 * A)
    cr.check_plan(c, p)
    g = cr.geom(c)
    if p.fmt:                               # the pack the launch reads has the size the restated layout has
        rows = c.Cout
        assert lib.call('ssg_pack_weights_split_bytes', rows, g.Kp, p.fmt) == cr.split_pack_bytes(rows, g.Kp, p.fmt)


def test_case_table_coverage():
    hit = cr.check_coverage()
    assert sorted(hit) == sorted(cr.REACHABLE_IDS)
    assert not cr.UNREACHABLE_IDS


SMALL = [c for c in cr.CASES if cr.geom(c).P <= 5000]


@pytest.mark.parametrize('c', SMALL, ids=_ids)
def test_integer_class_is_exact_in_fp32(c):
    ref = cr.conv_ref(c, cr.int_data(c))
    assert cr.int_class_is_exact(c, ref), float(np.nanmax(ref.magt))


def test_integer_class_bound_of_the_large_cases():
    """The cases too large to multiply out here: K |x| |w| + |bias| + |res| bounds the magnitude sum (no fused transform among them)."""
    for c in cr.CASES:
        g = cr.geom(c)
        if g.P > 5000:
            unit = 0.25 if ACT_LRELU in (c.act, c.bwd) else 1.0
            assert c.aff is None and (len(g.taps) * g.Cin * cr.irange(c, g) * 2 + 2000) / unit < 2 ** 24, c.name


# ----------------------------------------------------------------------------- the reference against fp64 torch
def _torch_ref(c, d):
    g = cr.geom(c)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=F64).transpose(0, 3, 1, 2)))
    X = t(cr.x_operand(c, d))[:, :g.cred_real]
    w = torch.from_numpy(d.w.astype(F64))
    if c.op == 'fwd':
        y = F.conv2d(X, w, None, c.stride, g.pad)
    else:
        y = torch.nn.grad.conv2d_input((c.N, c.ctot, c.H, c.W), w, X, c.stride, g.pad)[:, c.c_lo:c.c_lo + c.Cout]
    y = y.permute(0, 2, 3, 1).numpy()
    if c.bias:
        y = y + d.bias.astype(F64)
    if c.res:
        y = y + d.res.astype(F64)
    if c.bwd is not None:
        return y * cr.bwd_mask(c, d)[0]
    return cr.act64(y, c.act)


TORCH_CASES = ['reg0_c24_134', 'reg0_cat_s2', 'reg0_dgrad_slice', 'reg0_cls00', 'reg1_s2_cls', 'dmax3_50_cls_slice', 'k32_63_dgrad_slice', 'reg2_dgrad_cls11', 'dma22_cls01', 'dma20_cls11',
               'thin4in_c20', 'halo33_dgrad', 'splitk32_c208_136', 'parity_c16_64', 'parity_slice_ld', 'parity_even', 'k32_61_aff_lrelu',
               'k32_60_bwd_lrelu', 'k32_64_dgrad_20', 'dmax3_51_old_cls', 'dma21_s2_c32_40']


@pytest.mark.parametrize('name', TORCH_CASES)
def test_reference_matches_torch_fp64(name):
    c = cr.case(name); g = cr.geom(c)
    d = cr.rand_data(c)
    ref = cr.conv_ref(c, d)
    want = _torch_ref(c, d)
    assert want.shape == ref.out.shape
    w = ref.written
    if c.cls is None or c.cls == 'merge':
        assert w.all()
    else:                                   # one parity class: exactly the pixels of its phase
        ph = np.zeros(w.shape, dtype=bool); ph[:, c.cls[0]::2, c.cls[1]::2] = True
        assert np.array_equal(w, ph)
    assert np.isnan(ref.out[~w]).all()
    assert cr.worst_ratio((want - ref.out)[w], (1e-12 * ref.magt + 1e-300)[w]) <= 1
    ref2 = cr.conv_ref(c, d, elementwise=True)          # finite data: the non-finite path is the same sum
    assert cr.worst_ratio((ref2.out - ref.out)[w], (1e-12 * ref.magt + 1e-300)[w]) <= 1
    s1 = np.where(w, ref.acc + (d.bias.astype(F64) if c.bias else 0.0), 0.0).sum(axis=(0, 1, 2))
    if c.bwd is None:
        assert np.allclose(ref.colsum[0], s1, rtol=1e-12, atol=1e-9)


def test_nonfinite_reference_is_ieee():
    """One inf, one NaN, one 3.4e38 in x: the classes of conv_ref(elementwise) are those of a plain loop over the products."""
    c = cr.case('x3_41_c32_64'); g = cr.geom(c)
    d = cr.nonfinite_data(c, 'x')
    ref = cr.conv_ref(c, d, elementwise=True)
    X = cr.x_operand(c, d).astype(F64); Wt = cr.tap_weights(c, g, d.w).astype(F64)
    Xp = cr._padded(X, g, g.GH, g.GW, 1)
    with np.errstate(all='ignore'):
        acc = np.zeros((c.N, g.GH, g.GW, c.Cout))
        for t in range(9):
            xt = cr._tap_view(Xp, g.GH, g.GW, 1, g.taps[t][2], g.taps[t][3])
            for ci in range(g.Cin):
                acc += xt[..., ci:ci + 1] * Wt[t, ci]
    assert np.array_equal(cr.classes(acc), cr.classes(ref.acc))
    k = cr.classes(ref.acc)
    assert (k == 0).any() and (k == 3).any() and ((k == 1) | (k == 2)).any()


# ----------------------------------------------------------------------------- the packs
def test_restated_packs_are_consistent():
    rng = np.random.RandomState(3)
    w = cr._full(rng, (70, 24, 3, 3), 0.1)
    taps = [(ky, kx, ky - 1, kx - 1) for ky in range(3) for kx in range(3)]
    p1 = cr.pack_f32(w, 0, taps, 1, 24, 224)               # kmode 1: k = t Cred_pad + c, zero to Kp
    assert p1.shape == (70, 224) and p1[5, 3 * 24 + 7] == w[5, 7, 1, 0] and not p1[:, 216:].any()
    pt = cr.pack_f32(w, 1, taps, 1, 72, 656)               # transposed: rows = I, reduce over O (70 real of Cred_pad 72)
    assert pt.shape == (24, 656) and pt[7, 3 * 72 + 5] == w[5, 7, 1, 0] and not pt[:, 3 * 72 + 70:3 * 72 + 72].any()
    w = cr._full(rng, (128, 64, 3, 3), 0.1)
    p0 = cr.pack_f32(w, 0, taps, 0, 64, 576)               # kmode 0: k = (c / 16) 144 + t 16 + c % 16
    assert p0[9, 2 * 144 + 4 * 16 + 3] == w[9, 35, 1, 1]
    for bn in (64, 128):
        sp = cr.pack_split(p0[:100], bn)                    # 100 rows: the last tile is padded with zero rows
        assert sp.shape == (-(-100 // bn), 36, bn, 48) and sp.nbytes == cr.split_pack_bytes(100, 576, bn)
        row = 77; t, rl = divmod(row, bn); f = (rl >> 3) & 1
        tot = np.zeros(16)
        for p in range(3):
            for h in range(2):
                q = (2 * p + h) ^ f
                bits = sp[t, 5, rl, 8 * q:8 * q + 8].astype(np.uint32) << np.uint32(16)
                tot[8 * h:8 * h + 8] += bits.view(np.float32).astype(F64)
        assert np.array_equal(tot, p0[row, 80:96].astype(F64))
        assert not sp[-1, :, 100 - (sp.shape[0] - 1) * bn:].any()
    for code in (1016, 1032, 1064, 1128):
        bn = code - 1000
        R = bn if bn >= 64 else bn - 4
        sp = cr.pack_split_k32(p0[:R], code)
        assert sp.shape == (1, 18, bn // 16, 3, 64, 8) and sp.nbytes == cr.split_pack_bytes(R, 576, code)
        row, chunk32, tap, gq = R - 3, 1, 7, 2
        j, l = row // 16, (row % 16) + 16 * gq
        tot = sum((sp[0, chunk32 * 9 + tap, j, p, l].astype(np.uint32) << np.uint32(16)).view(np.float32).astype(F64) for p in range(3))
        c0 = chunk32 * 32 + gq * 8
        assert np.array_equal(tot, w[row, c0:c0 + 8, tap // 3, tap % 3].astype(F64))


# ----------------------------------------------------------------------------- the emulation, clean
STAT_CASES = [c for c in cr.CASES if c.stat]
ROWS_CASES = [c for c in cr.CASES if (c.bnpart or c.bwd is not None) and cr.geom(c).P <= 5000]


def _judge_layout(c, out, ref):
    """NaN exactly where nothing is written, zeros in the pad lanes of the written pixels."""
    w = ref.written[..., 0]
    nan_left = float(np.isnan(out[w][:, :c.Cout]).any(axis=1).mean()) if w.any() else 0.0
    return nan_left, bool(np.isnan(out[~w]).all()), bool((out[w][:, c.Cout:] == 0).all())


def _class_a(c, **defects):
    d = cr.int_data(c)
    ref = cr.conv_ref(c, d)
    out, rows, v32 = cr.emul(c, d, **defects)
    nan_left, untouched, pads = _judge_layout(c, out, ref)
    return cr.first_mismatch(out[..., :c.Cout], ref.out, ref.written), nan_left, untouched, pads


def _class_b(c, variant, **defects):
    g = cr.geom(c)
    d = cr.onehot_data(c, variant)
    ref = cr.conv_ref(c, d)
    out, _, _ = cr.emul(c, d, **defects)
    got = out[..., :c.Cout]
    assert np.count_nonzero(np.nan_to_num(ref.acc)) > 0
    if variant == 'full':
        return cr.judge(c, g, ref, got, cr.one_product_gate(c, g, ref))[0]
    want = ref.out.astype(F32).astype(F64)              # one rounding of p + bias: exact where there is no bias
    return 0.0 if cr.equal_values(got, want, ref.written) else np.inf


def _class_c(c, **defects):
    g = cr.geom(c)
    d = cr.rand_data(c)
    ref = cr.conv_ref(c, d)
    out, rows, v32 = cr.emul(c, d, **defects)
    r, ties = cr.judge(c, g, ref, out[..., :c.Cout], cr.hard_gate(c, g, ref))
    return r, ties, cr.rms((out[..., :c.Cout].astype(F64) - ref.out)[ref.written])


@pytest.mark.parametrize('c', STAT_CASES, ids=_ids)
def test_clean_emulation_passes_every_gate(c):
    msg, nan_left, untouched, pads = _class_a(c)
    assert msg is None and nan_left == 0 and untouched and pads, msg
    for variant in ('xpow2', 'wpow2', 'full'):
        r = _class_b(c, variant)
        if variant == 'full':
            print('EMUL %-24s (b) full %.3g' % (c.name, r))
        assert r <= 1, (variant, r)
    r, ties, e = _class_c(c)
    print('EMUL %-24s (c) hard %.3g  ties %.2g %%  rms %.3g' % (c.name, r, 100 * ties, e))
    assert r <= 1 and ties <= 0.01


@pytest.mark.parametrize('c', [c for c in SMALL if c.act != ACT_NONE or c.bwd is not None], ids=_ids)
def test_activation_ties_are_rare_in_the_reference(c):
    """The 1 % cap, on the reference alone: the share of elements whose pre-activation lies within the hard gate of 0 (or whose
    mask is decided within rounding).  The large grids draw from the same distributions."""
    g = cr.geom(c)
    d = cr.rand_data(c)
    ref = cr.conv_ref(c, d)
    gate = cr.hard_gate(c, g, ref)
    share = float((np.abs(ref.pre) <= gate)[ref.written].mean()) if c.act != ACT_NONE else cr.bwd_ties(c, d, ref)
    assert share <= 0.01, share


def _rows_ratios(c, d, out, rows, v32=None):
    """Totals of the rows against the column sums of the fp32 tensor they are statistics of."""
    ref = cr.conv_ref(c, d)
    src = out[..., :c.Cout] if v32 is None else v32
    want = cr.stats_of_output(c, d, src, ref.written)
    gates = cr.bwd_stats_gates(c, d, src, ref.written) if c.bwd is not None else cr.stats_gates(c, d, src)
    tot = rows.sum(axis=0)
    return cr.worst_ratio(tot[0] - want[0], gates[0]), cr.worst_ratio(tot[1] - want[1], gates[1])


@pytest.mark.parametrize('c', ROWS_CASES, ids=_ids)
def test_clean_emulation_passes_the_statistics_gates(c):
    d = cr.rand_data(c)
    out, rows, v32 = cr.emul(c, d)
    assert rows is not None and rows.shape == (cr.bnpart_rows(c), 2, c.Cout) and np.isfinite(rows).all()
    r1, r2 = _rows_ratios(c, d, out, rows)
    print('EMUL %-24s rows S1 %.3g S2 %.3g' % (c.name, r1, r2))
    assert r1 <= 1 and r2 <= 1
    # one pixel missing from the sums is seen: drop the last pixel's contribution from the last row
    g = cr.geom(c)
    last = out[-1, g.OH - 1, g.OW - 1, :c.Cout].astype(F64)
    rows2 = rows.copy()
    rows2[-1, 0] -= last
    rows2[-1, 1] -= last * last if c.bwd is None else last * (d.bx[-1, -1, -1].astype(F64) - d.bmean.astype(F64))
    r1, r2 = _rows_ratios(c, d, out, rows2)
    print('      one pixel less: S1 %.3g S2 %.3g' % (r1, r2))
    assert r1 > 1


# ----------------------------------------------------------------------------- planted defects
@pytest.mark.parametrize('name,defect', [
    ('halo32_c32_136', 'wrong_tap'), ('x3_41_c32_64', 'kykx_transposed'), ('halo33_dgrad', 'not_mirrored'),
    ('k32_61_w17_cat', 'in2_chunk_off'), ('x3_41_cat_192', 'in2_chunk_off'), ('k32_60_w33', 'drop_last_step'),
    ('splitk32_c176_40', 'drop_last_slab'), ('k32_60_aff_relu', 'xform_padding'), ('reg1_c24_40', 'lrelu_wrong_sign'),
    ('k32_60_bwd_relu', 'bwd_mask_from_grad'), ('parity_c16_64', 'parity_wrong_phase'), ('dma20_s2_c32_136', 'unit_stride_taps'),
    ('reg1_s2_cls', 'parity_wrong_phase')])
def test_indexing_defects_fail_class_a(name, defect):
    c = cr.case(name)
    msg, nan_left, untouched, pads = _class_a(c)
    assert msg is None and nan_left == 0 and untouched and pads, 'the clean emulation must pass first'
    msg, nan_left, untouched, pads = _class_a(c, **{defect: True})
    print('DEFECT %-22s %-20s %s; NaN left at %.0f %% of the pixels; untouched %s' % (name, defect, msg, 100 * nan_left, untouched))
    assert msg is not None or nan_left > 0 or not untouched


@pytest.mark.parametrize('defect', ['drop_last_col_tile', 'drop_last_row_tile'])
def test_unwritten_tiles_leave_nan(defect):
    c = cr.case('k32_60_w33')
    msg, nan_left, untouched, pads = _class_a(c, **{defect: True})
    print('DEFECT %-22s %-20s NaN left at %.0f %% of the pixels' % (c.name, defect, 100 * nan_left))
    assert nan_left > 0


def test_written_pad_lane_is_seen():
    c = cr.case('reg0_c24_134')
    assert _class_a(c)[3]
    msg, nan_left, untouched, pads = _class_a(c, pad_written=True)
    assert msg is None and not pads


def test_dropped_bf16_terms_fail_class_b_only():
    c = cr.case('k32_60_w33')
    for defect in ('drop_x3', 'drop_x2w2'):
        assert _class_a(c, **{defect: True})[0] is None          # (a): w is one bf16 term and x3 of these integers is zero
        r, ties, _ = _class_c(c, **{defect: True})               # (c): 2^-16 relative on every product is far inside K u32 mag
        print('DEFECT %-10s class (c) hard gate %.3g (passes)' % (defect, r))
        assert r <= 1
        r = _class_b(c, 'full', **{defect: True})
        print('DEFECT %-10s class (b) full %.3g' % (defect, r))
        assert r > 1
    assert _class_b(c, 'wpow2', drop_x3=True) > 1                 # x at full mantissa against a power of two: no longer exact
    assert _class_b(c, 'wpow2', drop_x2w2=True) <= 1              # w2 = 0 there: only `full` sees the missing product
    assert _class_b(c, 'xpow2', drop_x2w2=True) <= 1


def test_residual_before_the_statistics_fails_the_totals_gate():
    c = cr.case('halo32_bn')._replace(res=True)                    # the rows are judged against v = acc + bias (emul's v32)
    d = cr.rand_data(c)
    out, rows, v32 = cr.emul(c, d)
    r1, r2 = _rows_ratios(c, d, out, rows, v32)
    assert r1 <= 1 and r2 <= 1
    out, rows, v32 = cr.emul(c, d, res_before_stats=True)
    r1, r2 = _rows_ratios(c, d, out, rows, v32)
    print('DEFECT res_before_stats      rows S1 %.3g S2 %.3g' % (r1, r2))
    assert r1 > 1 and r2 > 1


def test_one_missing_term_fails_the_hard_gate_at_typical_elements():
    """K = 288: one product is ~ mag / K, the gate ~ K u32 mag = 2e-5 mag."""
    c = cr.case('k32_60_w33'); g = cr.geom(c)
    d = cr.rand_data(c)
    ref = cr.conv_ref(c, d)
    w2 = d.w.copy(); w2[:, 7, 1, 1] = 0
    short = cr.conv_ref(c, d._replace(w=w2))
    live = ref.pre > 0                                            # the case has a ReLU: an element it zeroes cannot show a missing term
    over = (np.abs(short.out - ref.out) > cr.hard_gate(c, g, ref))[live]
    print('one term of %d missing: %.1f %% of the elements the ReLU passes exceed the hard gate' % (288, 100 * over.mean()))
    assert over.mean() > 0.9


def test_split_is_exact_and_low_terms_are_present():
    rng = np.random.RandomState(5)
    a = cr._full(rng, (4096,), 0.3)
    a1, a2, a3 = cr.split3(a)
    assert np.array_equal(a1.astype(F64) + a2.astype(F64) + a3.astype(F64), a.astype(F64))
    assert np.count_nonzero(a3) > 0.95 * a.size
