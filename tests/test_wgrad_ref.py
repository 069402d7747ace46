"""CPU rehearsal of tests/wgrad_ref.py, the oracle of tests/test_wgrad_gpu.py, before a GPU sees it:

* the restated make_plan equals ssg_conv2d_wgrad_kernel_id, ssg_conv2d_wgrad_workspace_bytes / (ntaps Cin Cout 4) and
  ssg_conv2d_wgrad_in_affine_ok of the built library at every case (dummy addresses, nothing launched), the case table reaches
  every reachable kernel id x feature (check_coverage), and the integer class stays below 2^24 at every case;
* the fp64 reference agrees with fp64 torch (F.conv2d and autograd);
* the float32 emulation passes every gate of classes (a), (b) and (c) at the cases it is run on;
* each of the twelve planted defects fails the gate it is meant for: indexing defects fail class (a), the dropped bf16 terms
  fail class (b); one missing pixel of ~1000 fails the hard gate of class (c) at most elements.

Defect -> gate (the case it is shown on; what the gate reports, as printed by this module with -s):

     1 last column strip dropped (k32_w33_h12)                           class (a): 24490 of 36864 elements differ
     2 one-column ragged strip read one pixel too far (k32_w33_h12)     class (a): 24509 of 36864
     3 window not reloaded at a mid-strip slab start (k32_w33_h12)      class (a): 12267 of 36864 (the taps of the row above)
     4 last slab dropped (k32_w33_h12, dma_slabs_1)                      class (a): 24435 of 36864, 639 of 640
     5 in2's channels one block further (k32_cat)                        class (a): 36845 of 73728 (in2's half)
     6 ky / kx transposed (halo_64x48_w33)                               class (a): 18418 of 27648 (the six off-diagonal taps)
     7 pad channels written (reg_cat_ld)                                 class (a): 414 of 4752, and the guard behind dw
     8 input transform applied to padding pixels (k32_aff_relu)          class (a): 32448 of 36864 (all but the centre tap)
     9 leaky slope on the wrong sign (k32_aff_lrelu)                     class (a): 36835 of 36864
    10 third bf16 term of x dropped (k32_w33_h12)                        class (b): dout a power of two is no longer exact, `full` at
                                                                         14 x the gate.  Classes (a) and (c) pass (hard gate 0.013).
    11 x2 d2 product dropped (k32_w33_h12)                               class (b) `full` only, 27 x the gate; (a) and (c) pass (0.015)
    12 stride-2 taps read at unit stride (dma_s2_15x17)                  class (a): 9206 of 9216

The clean emulation at the twenty-one `stat` cases: class (a) exact, class (b) exact with a power-of-two operand and 0.14 .. 0.20
(split routes) / 0.89 .. 0.995 (fp32 routes) of the product gate at full mantissas, class (c) at most 0.12 of the hard gate.  With
one pixel of 792 missing, 92 % of the elements of k32_w33_h12 exceed the hard gate.
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import wgrad_ref as wr
from wgrad_ref import F64

A = 1 << 32                                 # dummy addresses: 16-byte aligned, distinct, never dereferenced


@pytest.fixture(scope='module')
def lib(pkg):
    yield pkg._lib
    pkg._lib.call('ssg_wgrad_set_k32_mode', 1)


def _ids(c):
    return c.name


# ----------------------------------------------------------------------------- restatement and coverage
@pytest.mark.parametrize('c', wr.CASES, ids=_ids)
def test_plan_restatement_matches_library(lib, c):
    lib.call('ssg_wgrad_set_k32_mode', c.k32)
    d = wr.fill_desc(lib.WgradDesc(), c, A, 2 * A, 3 * A, 4 * A, scale=5 * A, shift=6 * A)
    g = wr.geom(c); p = wr.make_plan(c)
    assert lib.call('ssg_conv2d_wgrad_kernel_id', ctypes.byref(d)) == p.kid
    ws = lib.call('ssg_conv2d_wgrad_workspace_bytes', ctypes.byref(d))
    assert ws == wr.workspace_bytes(c) and ws // (g.ntaps * g.Cin * c.Cout * 4) == p.splits
    assert bool(lib.call('ssg_conv2d_wgrad_in_affine_ok', ctypes.byref(d))) == (p.aff_ok and c.C2 == 0)
    if c.aff is None:                       # the same descriptor with a transform attached: only the k32 route takes one
        d.in_scale = 5 * A; d.in_shift = 6 * A; d.in_act = 1
        assert bool(lib.call('ssg_conv2d_wgrad_in_affine_ok', ctypes.byref(d))) == (p.kid == 60 and c.C2 == 0)


def test_case_table_coverage():
    hit = wr.check_coverage()
    assert sorted(hit) == sorted(wr.REACHABLE_IDS)
    assert not set(wr.REACHABLE_IDS) & set(wr.UNREACHABLE_IDS)


@pytest.mark.parametrize('c', [c for c in wr.CASES if wr.geom(c).P <= 5000], ids=_ids)
def test_integer_class_is_exact_in_fp32(c):
    x1, x2, d, sc, sh = wr.int_data(c)
    _, mag = wr.wgrad_ref(c, x1, x2, d, sc, sh)
    assert wr.int_class_is_exact(c, mag), float(mag.max())


def test_integer_class_bound_of_the_large_cases():
    """The cases too large to multiply out here: P |x| |d| bounds the magnitude sum."""
    for c in wr.CASES:
        if wr.geom(c).P > 5000:
            assert c.aff is None and wr.geom(c).P * c.irange * c.irange < 2 ** 24, c.name


# ----------------------------------------------------------------------------- the reference against fp64 torch
@pytest.mark.parametrize('name', ['k32_cat_ld', 'dma_cat_s2', 'reg_c24_s2', 'w4in_c96_1x1', 'halo_w1_h9', 'k32_aff_lrelu'])
def test_reference_matches_torch_fp64(name):
    c = wr.case(name); g = wr.geom(c)
    x1, x2, d, sc, sh = wr.rand_data(c)
    X = torch.from_numpy(wr.x_operand(c, x1, x2, sc, sh).astype(F64).transpose(0, 3, 1, 2).copy())
    w = torch.zeros((c.Cout, g.Cin, c.k, c.k), dtype=torch.float64, requires_grad=True)
    y = F.conv2d(X, w, stride=c.stride, padding=g.pad)
    assert tuple(y.shape[2:]) == (g.GH, g.GW)
    y.backward(torch.from_numpy(d.astype(F64).transpose(0, 3, 1, 2).copy()))
    ref, mag = wr.wgrad_ref(c, x1, x2, d, sc, sh)
    assert wr.worst_ratio(w.grad.numpy()[:, :g.cin_real] - ref, 1e-12 * mag + 1e-300) <= 1
    ref2, mag2 = wr.wgrad_ref(c, x1, x2, d, sc, sh, elementwise=True)
    assert wr.worst_ratio(ref2 - ref, 1e-12 * mag + 1e-300) <= 1 and wr.worst_ratio(mag2 - mag, 1e-12 * mag + 1e-300) <= 1


# ----------------------------------------------------------------------------- the emulation, clean
STAT_CASES = [c for c in wr.CASES if c.stat]


def _emul(c, data, **defects):
    return wr.emul_dw(c, wr.emul(c, *data, **defects))


@pytest.mark.parametrize('c', STAT_CASES, ids=_ids)
def test_clean_emulation_passes_every_gate(c):
    g = wr.geom(c); split = wr.make_plan(c).kid in wr.SPLIT_IDS
    data = wr.int_data(c)
    dw, guard = _emul(c, data)
    ref, _ = wr.wgrad_ref(c, *data)
    assert guard and wr.equal_values(dw, ref), wr.first_mismatch(dw, ref)                           # (a)
    for variant in ('dpow2', 'xpow2', 'full'):                                                      # (b)
        data = wr.onehot_data(c, variant)
        dw, _ = _emul(c, data)
        ref, _ = wr.wgrad_ref(c, *data)
        assert np.count_nonzero(ref) > 0
        if variant == 'full':
            r = wr.worst_ratio(dw.astype(F64) - ref, wr.product_gate(ref, split))
            print('EMUL %-20s (b) full %.3g' % (c.name, r))
            assert r <= 1
        else:
            assert wr.equal_values(dw, ref), (variant, wr.first_mismatch(dw, ref))
    data = wr.rand_data(c)                                                                          # (c)
    dw, _ = _emul(c, data)
    ref, mag = wr.wgrad_ref(c, *data)
    r = wr.worst_ratio(dw.astype(F64) - ref, wr.hard_gate(ref, mag, g.P, split))
    print('EMUL %-20s (c) hard %.3g  rms %.3g of rms(ref) %.3g' % (c.name, r, wr.rms(dw.astype(F64) - ref), wr.rms(ref)))
    assert r <= 1


def test_one_missing_pixel_fails_the_hard_gate_at_typical_elements():
    """P = 792: one pixel's term is ~ mag / P, the gate ~ P u32 mag = 5e-5 mag."""
    c = wr.case('k32_w33_h12'); g = wr.geom(c)
    x1, x2, d, sc, sh = wr.rand_data(c)
    ref, mag = wr.wgrad_ref(c, x1, x2, d, sc, sh)
    d2 = d.copy(); d2[1, 5, 20] = 0
    short, _ = wr.wgrad_ref(c, x1, x2, d2, sc, sh)
    over = np.abs(short - ref) > wr.hard_gate(ref, mag, g.P, True)
    print('one pixel of %d missing: %.1f %% of the elements exceed the hard gate' % (g.P, 100 * over.mean()))
    assert over.mean() > 0.9


# ----------------------------------------------------------------------------- planted defects
def _class_a_fails(name, **defect):
    c = wr.case(name)
    data = wr.int_data(c)
    ref, _ = wr.wgrad_ref(c, *data)
    clean, guard = _emul(c, data)
    assert guard and wr.equal_values(clean, ref), 'the clean emulation must pass first'
    dw, guard = _emul(c, data, **defect)
    msg = wr.first_mismatch(dw, ref)
    print('DEFECT %-20s %-18s %s%s' % (name, list(defect)[0], msg, '' if guard else '; guard behind dw overwritten'))
    return (not wr.equal_values(dw, ref)), guard


@pytest.mark.parametrize('name,defect', [
    ('k32_w33_h12', 'drop_last_strip'), ('k32_w33_h12', 'ragged_too_far'), ('k32_w33_h12', 'stale_window'),
    ('k32_w33_h12', 'drop_last_slab'), ('dma_slabs_1', 'drop_last_slab'), ('k32_cat', 'in2_block_off'),
    ('halo_64x48_w33', 'kykx_transposed'), ('reg_cat_ld', 'pad_written'), ('k32_aff_relu', 'xform_padding'),
    ('k32_aff_lrelu', 'lrelu_wrong_sign'), ('dma_s2_15x17', 'unit_stride_taps')])
def test_indexing_defects_fail_class_a(name, defect):
    fails, guard = _class_a_fails(name, **{defect: True})
    assert fails
    if defect == 'pad_written':
        assert not guard


def test_dropped_bf16_terms_fail_class_b_only():
    c = wr.case('k32_w33_h12'); g = wr.geom(c)
    for defect in ('drop_x3', 'drop_x2d2'):
        data = wr.int_data(c)                                        # (a): integers are single bf16 terms, the defect is invisible
        ref, _ = wr.wgrad_ref(c, *data)
        assert wr.equal_values(_emul(c, data, **{defect: True})[0], ref)
        data = wr.rand_data(c)                                       # (c): 2^-16 relative on every product is far inside P u32 mag
        ref, mag = wr.wgrad_ref(c, *data)
        r = wr.worst_ratio(_emul(c, data, **{defect: True})[0].astype(F64) - ref, wr.hard_gate(ref, mag, g.P, True))
        print('DEFECT %-10s class (c) hard gate %.3g (passes)' % (defect, r))
        assert r <= 1
        data = wr.onehot_data(c, 'full')                             # (b)
        ref, _ = wr.wgrad_ref(c, *data)
        r = wr.worst_ratio(_emul(c, data, **{defect: True})[0].astype(F64) - ref, wr.product_gate(ref, True))
        print('DEFECT %-10s class (b) full %.3g' % (defect, r))
        assert r > 1
    data = wr.onehot_data(c, 'dpow2')
    ref, _ = wr.wgrad_ref(c, *data)
    assert not wr.equal_values(_emul(c, data, drop_x3=True)[0], ref)


def test_split_is_exact_and_low_terms_are_present():
    rng = np.random.RandomState(5)
    a = wr._full(rng, (4096,), 0.3)
    a1, a2, a3 = wr.split3(a)
    assert np.array_equal(a1.astype(F64) + a2.astype(F64) + a3.astype(F64), a.astype(F64))
    assert np.count_nonzero(a3) > 0.95 * a.size and np.count_nonzero(a2) > 0.95 * a.size
    assert np.all(np.abs(a2) <= 2.0 ** -8 * np.abs(a)) and np.all(np.abs(a3) <= 2.0 ** -16 * np.abs(a))
