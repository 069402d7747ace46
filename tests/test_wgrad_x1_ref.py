"""CPU rehearsal of the gates of tests/test_wgrad_x1_gpu.py: wgrad_x1_ref.emul -- the bf16x1 weight gradient in float32 with the
kernel's slab partition -- passes every gate at the GPU test's cases, and each planted defect fails one.  The restated plan and
predicate are pinned to the built library's host queries (no GPU needed: they launch nothing)."""
import ctypes as C_

import numpy as np
import pytest

import wgrad_ref as wr
import wgrad_x1_ref as xr
from wgrad_ref import F64


def _ratios(c, dw, data):
    ref_r, mag_r = xr.ref_rounded(c, data)
    ref_e, mag_e = xr.ref_exact(c, data)
    return (wr.worst_ratio(dw.astype(F64) - ref_r, xr.gate_rounded(c, ref_r, mag_r)),
            wr.worst_ratio(dw.astype(F64) - ref_e, xr.gate_exact(c, ref_r, mag_r, mag_e)))


@pytest.mark.parametrize('c', xr.CASES, ids=lambda c: c.name)
def test_emulation_passes_every_gate(c):
    data = wr.int_data(c)
    ref, mag = wr.wgrad_ref(c, *data)
    assert wr.int_class_is_exact(c, mag)
    assert wr.equal_values(xr.emul(c, data), ref)
    data = wr.onehot_data(c, 'full')
    assert wr.equal_values(xr.emul(c, data), xr.ref_rounded(c, data)[0])
    data = wr.rand_data(c)
    r_rounded, r_exact = _ratios(c, xr.emul(c, data), data)
    assert r_rounded <= 1 and r_exact <= 1, (r_rounded, r_exact)


DEFECTS = [dict(unrounded_x=True), dict(truncate=True), dict(drop_tap=5), dict(swap_planes=True), dict(drop_last_slab=True)]


@pytest.mark.parametrize('defect', DEFECTS, ids=lambda d: next(iter(d)))
def test_each_planted_defect_fails_a_gate(defect):
    c = xr.case(xr.RAGGED)
    failed = []
    data = wr.int_data(c)
    if not wr.equal_values(xr.emul(c, data, **defect), wr.wgrad_ref(c, *data)[0]):
        failed.append('integers')
    data = wr.onehot_data(c, 'full')
    if not wr.equal_values(xr.emul(c, data, **defect), xr.ref_rounded(c, data)[0]):
        failed.append('one-hot')
    data = wr.rand_data(c)
    r_rounded, r_exact = _ratios(c, xr.emul(c, data, **defect), data)
    if r_rounded > 1:
        failed.append('rounded bound')
    if r_exact > 1:
        failed.append('exact bound')
    print(defect, failed, r_rounded, r_exact)
    assert failed, 'no gate sees %s' % defect
    # integers are bf16 numbers: rounding defects must be seen by the full-mantissa classes, indexing defects by the integers too
    if 'drop_tap' in defect or 'swap_planes' in defect or 'drop_last_slab' in defect:
        assert 'integers' in failed
    else:
        assert 'one-hot' in failed and 'rounded bound' in failed


def test_bound_constants():
    # unit roundoff 2^-9 per operand: 1 + 2^-8 is a tie between 1 and 1 + 2^-7 and goes to even
    one = np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8], dtype=np.float32)
    assert list(wr.bf16_rne(one)) == [1.0, 1.0 + 2.0 ** -6]
    assert xr.BOUND == (1 + 2.0 ** -9) ** 2 - 1
    # 3.4e38 rounds to infinity in bf16, 3.39e38 does not
    import torch
    v = torch.tensor([3.4e38, 3.39e38]).bfloat16().float()
    assert torch.isinf(v[0]) and torch.isfinite(v[1])


def _desc(lib, c):
    return wr.fill_desc(lib.WgradDesc(), c, 16, 16 if c.C2 else None, 16, 16)


def test_restated_plan_matches_the_library(pkg):
    lib = pkg._lib
    for c in xr.CASES:
        d = _desc(lib, c)
        assert lib.call('ssg_conv2d_wgrad_bf16x1_ok', C_.byref(d)) == 1
        assert lib.call('ssg_conv2d_wgrad_bf16x1_kernel_id', C_.byref(d)) == xr.KERNEL_ID
        assert lib.call('ssg_conv2d_wgrad_bf16x1_workspace_bytes', C_.byref(d)) == xr.workspace_bytes(c)
    # the flagship's shapes: slabs of at most 128 steps
    for c in (wr._c('b512', 16, 512, 512, 64, 0, 64), wr._c('b256', 16, 256, 256, 128, 128, 128), wr._c('b32', 16, 32, 32, 1024, 0, 1024)):
        d = _desc(lib, c)
        assert lib.call('ssg_conv2d_wgrad_bf16x1_workspace_bytes', C_.byref(d)) == xr.workspace_bytes(c)
        assert xr.plan(c)[4] <= xr.MAX_ROWS


def test_refused_descriptors_answer_zero(pkg):
    lib = pkg._lib
    for c in (wr._c('s2', 1, 8, 40, 64, 0, 64, stride=2), wr._c('k1', 1, 4, 40, 64, 0, 64, k=1), wr._c('c32', 1, 4, 40, 32, 0, 64),
              wr._c('w16', 1, 4, 16, 64, 0, 64), wr._c('co32', 1, 4, 40, 64, 0, 32), wr._c('real', 1, 4, 40, 64, 0, 64, cin_real=61)):
        assert not xr.ok(c)
        d = _desc(lib, c)
        assert lib.call('ssg_conv2d_wgrad_bf16x1_ok', C_.byref(d)) == 0
        assert lib.call('ssg_conv2d_wgrad_bf16x1_kernel_id', C_.byref(d)) == -1
        assert lib.call('ssg_conv2d_wgrad_bf16x1_workspace_bytes', C_.byref(d)) == 0
        assert lib.load().ssg_conv2d_wgrad_bf16x1_f32(C_.byref(d), None) != 0     # a status before any launch (no GPU here)
    c = xr.case('x1_w17')
    d = _desc(lib, c)
    d.in_scale = 16; d.in_shift = 16
    assert lib.call('ssg_conv2d_wgrad_bf16x1_ok', C_.byref(d)) == 0
    # ssg_conv2d_wgrad_f32's plan never names the new kernel
    d = _desc(lib, c)
    assert lib.call('ssg_conv2d_wgrad_kernel_id', C_.byref(d)) == 60
