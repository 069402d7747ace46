"""CPU rehearsal of tests/test_wgrad_s2_x1_gpu.py (no GPU): the case table's own conditions, and the gates of that test applied to
wgrad_s2_x1_ref.emul -- the float32 emulation of wgrad_s2_k32_x1_kernel's arithmetic and addressing passes every gate at every
case, and each planted defect fails at least one."""
import numpy as np
import pytest

import wgrad_ref as wr
import wgrad_s2_x1_ref as sr
from wgrad_ref import F64

DEFECTS = ['unit_stride_taps', 'odd_off_by_one', 'swap_planes', 'row_off_by_one', 'right_pad_nonzero', 'bottom_pad_nonzero',
           'drop_ragged_step']
_REF = {}


def _ref(c, cls):
    """(data, fp64 references) of a case and data class, computed once."""
    key = (c.name, cls)
    if key not in _REF:
        if cls == 'int':
            data = wr.int_data(c)
            _REF[key] = (data,) + wr.wgrad_ref(c, *data)
        elif cls in ('interior', 'edge'):
            data = sr.onehot_data(c, cls)
            _REF[key] = (data,) + sr.ref_rounded(c, data)
        else:
            data = wr.rand_data(c)
            _REF[key] = (data,) + sr.ref_rounded(c, data) + sr.ref_exact(c, data)
    return _REF[key]


def gates(c, dw_of):
    """Names of the gates of the GPU test that `dw_of(data)` fails at case c."""
    failed = []
    data, ref, _ = _ref(c, 'int')
    if not wr.equal_values(dw_of(data), ref):
        failed.append('int')
    for where in ('interior', 'edge'):
        data, ref1, _ = _ref(c, where)
        if not wr.equal_values(dw_of(data), ref1):
            failed.append('onehot_' + where)
    data, ref_r, mag_r, ref_e, mag_e = _ref(c, 'rand')
    dw = dw_of(data).astype(F64)
    if wr.worst_ratio(dw - ref_r, sr.gate_rounded(c, ref_r, mag_r)) > 1:
        failed.append('rounded')
    if wr.worst_ratio(dw - ref_e, sr.gate_exact(c, ref_r, mag_r, mag_e)) > 1:
        failed.append('exact')
    return failed


def test_case_table():
    assert [(c.N, c.H, c.W, c.C1, c.Cout) for c in sr.CASES] == [(1, 5, 33, 64, 64), (1, 4, 34, 64, 128), (1, 6, 79, 128, 64),
                                                                  (1, 2, 64, 64, 64), (3, 37, 66, 64, 128), (1, 4, 34, 64, 64)]
    for c in sr.CASES:
        assert sr.ok(c), c.name
        g = wr.geom(c)
        assert (g.GH, g.GW) == ((c.H + 1) // 2, (c.W + 1) // 2)
        _, mag = wr.wgrad_ref(c, *wr.int_data(c))
        assert wr.int_class_is_exact(c, mag), c.name
        assert sr.workspace_bytes(c) == sr.plan(c)[5] * 9 * c.C1 * c.Cout * 4
    assert {sr.kernel_id(c) for c in sr.CASES} == {81, 82}
    c = sr.case(sr.SLABS)
    g = wr.geom(c)
    _, _, _, steps, sps, splits = sr.plan(c)
    assert splits > 1 and steps % sps != 0
    assert any((z * sps) % g.GH for z in range(1, splits)), 'no slab boundary inside a strip'
    assert g.GW % sr.KP == 1                                             # the last step of the ragged last slab is a one-column step
    c = sr.case('s2_ld')
    g = wr.geom(c)
    assert g.ld1 > c.C1 and g.ldd > c.Cout
    # refusals the GPU test makes: each by one condition
    for bad in (wr._c('s1', 1, 8, 40, 64, 0, 64), wr._c('k1', 1, 4, 40, 64, 0, 64, k=1, stride=2), wr._c('c32', 1, 4, 40, 32, 0, 64, stride=2),
                wr._c('o32', 1, 4, 40, 64, 0, 32, stride=2), wr._c('w32', 1, 4, 32, 64, 0, 64, stride=2), wr._c('cat', 1, 4, 40, 64, 64, 64, stride=2)):
        assert not sr.ok(bad), bad.name


def test_onehot_pixels_hit_padding():
    """The 'edge' pixel's window reaches the right / bottom padding where W / H is odd; the 'interior' one never does."""
    for c in sr.CASES:
        g = wr.geom(c)
        d = sr.onehot_data(c, 'edge')[2]
        n, oy, ox = [int(v[0]) for v in np.nonzero(np.abs(d).sum(axis=-1))]
        assert (oy, ox) == (g.GH - 1, g.GW - 1)
        assert (2 * ox + 1 == c.W) == (c.W % 2 == 1) and (2 * oy + 1 == c.H) == (c.H % 2 == 1)
        d = sr.onehot_data(c, 'interior')[2]
        n, oy, ox = [int(v[0]) for v in np.nonzero(np.abs(d).sum(axis=-1))]
        assert 2 * ox + 1 < c.W and 2 * ox - 1 >= 0


@pytest.mark.parametrize('c', sr.CASES, ids=lambda c: c.name)
def test_emulation_passes_every_gate(c):
    assert gates(c, lambda data: sr.emul(c, data)) == []


@pytest.mark.parametrize('defect', DEFECTS)
def test_planted_defect_fails_a_gate(defect):
    caught = {}
    for c in sr.CASES:
        f = gates(c, lambda data: sr.emul(c, data, **{defect: True}))
        if f:
            caught[c.name] = f
    print('DEFECT %-20s %s' % (defect, caught))
    assert caught, 'no gate at any case notices %s' % defect


def test_nonfinite_data_has_every_class():
    c = sr.case(sr.NONFINITE_CASE)
    data = sr.nonfinite_data(c)
    with np.errstate(all='ignore'):
        ref, _ = wr.wgrad_ref(c, *data, elementwise=True)
        want = wr.classes(ref.astype(np.float32))
    assert (want == 0).any() and (want == 1).any() and (want == 2).any() and (want == 3).any()
