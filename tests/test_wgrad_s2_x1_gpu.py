"""ssg_conv2d_wgrad_bf16x1_s2_f32 (csrc/conv_wgrad_s2_k32_x1.hip, kernel ids 81 / 82) against tests/wgrad_s2_x1_ref.py, through the
C-ABI.  tests/test_wgrad_s2_x1_ref.py rehearses the gates on the CPU: the float32 emulation passes them at these cases, each
planted defect fails one.

Per case of wgrad_s2_x1_ref.CASES:
  (a) integer operands in [-3, 3]: every product and sum is exact in bf16 and fp32 -> bit equality with fp64;
  (b) one non-zero dout pixel, full-mantissa operands, once at an interior pixel and once at the last row / last column (the
      padding taps): every element is f32(bf16(x) * bf16(dout)), bit for bit;
  (c) full-mantissa operands: (P + 2) u32 mag + u32 |ref| against fp64 on the rounded operands, and that plus
      (2^-8 + 2^-18) sum |x| |dout| against fp64 on the operands as given (P = output pixels).
Every launch: dw and the workspace NaN-filled between poisoned bands, the workspace exactly the queried size and the restated
plan's, two runs with the same bits, the kernel id 81 / 82 by Cout % 128.  Non-finite x and dout: every element has the class the
fp32-class kernel (ssg_conv2d_wgrad_f32, id 50 / 51) gives on the same buffers.  Host refusals return a status and launch nothing."""
import ctypes as C_

import numpy as np
import pytest
import torch

import wgrad_ref as wr
import wgrad_s2_x1_ref as sr
from test_wgrad_x1_gpu import SSG_EINVAL, _Launch
from wgrad_ref import F64

pytestmark = pytest.mark.gpu

ENTRY = 'ssg_conv2d_wgrad_bf16x1_s2'
IDS_RUN = set()


def _launch(pkg, dev, c, data):
    lib = pkg._lib
    L = _Launch(lib, dev, c, data, entry=ENTRY)
    assert lib.call(ENTRY + '_ok', C_.byref(L.desc)) == 1
    kid = lib.call(ENTRY + '_kernel_id', C_.byref(L.desc))
    assert kid == sr.kernel_id(c) == (81 if c.Cout % 128 == 0 else 82)
    IDS_RUN.add(kid)
    assert L.ws_bytes == sr.workspace_bytes(c), 'the library plans %d workspace bytes, the restated plan %d' % (L.ws_bytes, sr.workspace_bytes(c))
    # the other two routes keep refusing / ignoring this descriptor
    assert lib.call('ssg_conv2d_wgrad_bf16x1_ok', C_.byref(L.desc)) == 0
    assert lib.call('ssg_conv2d_wgrad_kernel_id', C_.byref(L.desc)) in sr.FP32_IDS
    return L


@pytest.mark.parametrize('c', sr.CASES, ids=lambda c: c.name)
def test_wgrad_s2_x1_case(pkg, dev, c):
    g = wr.geom(c)
    assert sr.ok(c)
    # (a) integers in [-3, 3]: exact
    data = wr.int_data(c)
    ref, mag = wr.wgrad_ref(c, *data)
    assert wr.int_class_is_exact(c, mag)
    dw = _launch(pkg, dev, c, data).run()
    assert wr.equal_values(dw, ref), 'integer operands: %s' % wr.first_mismatch(dw, ref)
    # (b) one non-zero dout pixel: each element one exact product of the rounded operands
    for where in ('interior', 'edge'):
        data = sr.onehot_data(c, where)
        ref1, _ = sr.ref_rounded(c, data)
        dw1 = _launch(pkg, dev, c, data).run()
        assert np.count_nonzero(ref1) > ref1.size // 4
        assert wr.equal_values(dw1, ref1), 'one-hot dout pixel (%s): %s' % (where, wr.first_mismatch(dw1, ref1))
    # (c) full mantissas: both bounds
    data = wr.rand_data(c)
    ref_r, mag_r = sr.ref_rounded(c, data)
    ref_e, mag_e = sr.ref_exact(c, data)
    dw = _launch(pkg, dev, c, data).run()
    r_rounded = wr.worst_ratio(dw.astype(F64) - ref_r, sr.gate_rounded(c, ref_r, mag_r))
    r_exact = wr.worst_ratio(dw.astype(F64) - ref_e, sr.gate_exact(c, ref_r, mag_r, mag_e))
    print('RATIO id=%d %-16s P=%d splits=%d rounded=%.3g exact=%.3g' % (sr.kernel_id(c), c.name, g.P, sr.plan(c)[5], r_rounded, r_exact))
    assert r_rounded <= 1 and r_exact <= 1, (r_rounded, r_exact)


def test_nonfinite_operands(pkg, dev):
    c = sr.case(sr.NONFINITE_CASE)
    data = sr.nonfinite_data(c)
    dw = _launch(pkg, dev, c, data).run()
    # the fp32-class kernel on the same operands
    L32 = _Launch(pkg._lib, dev, c, data, entry='ssg_conv2d_wgrad')
    assert pkg._lib.call('ssg_conv2d_wgrad_kernel_id', C_.byref(L32.desc)) in sr.FP32_IDS
    dw32 = L32.run()
    got, got32 = wr.classes(dw), wr.classes(dw32)
    assert (got32 == 0).any() and (got32 == 1).any() and (got32 == 2).any() and (got32 == 3).any()
    bad = np.argwhere(got != got32)
    assert not len(bad), '%d elements in another class than the fp32 kernel, first %s: got %r, fp32 kernel %r' % (
        len(bad), tuple(bad[0]), dw[tuple(bad[0])], dw32[tuple(bad[0])])
    # 3.4e38 in x against zero dout (input channel 3), in dout against zero x (output channel 2): finite in fp32 (3.4e38 * 0 = 0),
    # NaN with a bf16 infinity -- the guard's case.  Looked at on the channels of the other operand that hold no planted value.
    co_clean = np.setdiff1d(np.arange(c.Cout), [(2 + 7 * i) % c.Cout for i in range(5)] + [(4 + 9 * i) % c.Cout for i in range(5)])
    ci_clean = np.setdiff1d(np.arange(c.C1), [(3 + 11 * i) % c.C1 for i in range(5)] + [(5 + 13 * i) % c.C1 for i in range(5)])
    assert np.isfinite(dw[co_clean, 3]).all() and np.isfinite(dw[2][ci_clean]).all()


def _refused(lib, L):
    L.dw.fill(); L.ws.fill()
    assert lib.call(ENTRY + '_ok', C_.byref(L.desc)) == 0
    assert lib.call(ENTRY + '_kernel_id', C_.byref(L.desc)) == SSG_EINVAL
    assert lib.call(ENTRY + '_workspace_bytes', C_.byref(L.desc)) == 0
    L.desc.ws_bytes = 1 << 30                      # not the workspace check: the shape is what is refused
    rc = L.status()
    torch.cuda.synchronize()
    assert rc == SSG_EINVAL, 'status %d' % rc
    assert b'wgrad bf16x1 s2' in lib.load().ssg_last_error()
    assert bool(torch.isnan(L.dw.body()).all().item()) and L.dw.intact(), 'a refused call wrote dw'
    assert bool(torch.isnan(L.ws.body()).all().item()), 'a refused call wrote the workspace'


def test_host_refusals(pkg, dev):
    lib = pkg._lib
    for c in (wr._c('s1', 1, 8, 40, 64, 0, 64), wr._c('k1', 1, 4, 40, 64, 0, 64, k=1, stride=2),
              wr._c('c32', 1, 4, 40, 32, 0, 64, stride=2), wr._c('o32', 1, 4, 40, 64, 0, 32, stride=2),
              wr._c('w32', 1, 4, 32, 64, 0, 64, stride=2), wr._c('cat', 1, 4, 40, 64, 64, 64, stride=2)):
        assert not sr.ok(c)
        _refused(lib, _Launch(lib, dev, c, wr.int_data(c), entry=ENTRY))
    c = sr.case('s2_w33_h5')
    L = _Launch(lib, dev, c, wr.int_data(c), entry=ENTRY)
    sc = torch.ones(c.C1, device=dev); sh = torch.zeros(c.C1, device=dev)
    L.desc.in_scale = sc.data_ptr(); L.desc.in_shift = sh.data_ptr()
    _refused(lib, L)
    L = _launch(pkg, dev, c, wr.int_data(c))
    L.desc.ws_bytes = L.ws_bytes - 1               # workspace one byte short
    L.dw.fill(); L.ws.fill()
    assert L.status() == SSG_EINVAL
    torch.cuda.synchronize()
    assert b'wgrad bf16x1 s2' in lib.load().ssg_last_error()
    assert bool(torch.isnan(L.dw.body()).all().item()) and bool(torch.isnan(L.ws.body()).all().item())
    L = _launch(pkg, dev, c, wr.int_data(c))        # and the untouched descriptor still runs
    ref, _ = wr.wgrad_ref(c, *wr.int_data(c))
    assert wr.equal_values(L.run(), ref)
    assert lib.call('ssg_conv2d_wgrad_bf16x1_ok', C_.byref(L.desc)) == 0       # the stride-1 entry still refuses stride 2


def test_both_kernel_ids_ran(pkg, dev):
    """Over the file both instantiations have run (this test runs one case of each itself when selected alone)."""
    for name in ('s2_w33_h5', 's2_w34_h4_c128'):
        c = sr.case(name)
        data = wr.int_data(c)
        ref, _ = wr.wgrad_ref(c, *data)
        assert wr.equal_values(_launch(pkg, dev, c, data).run(), ref)
    assert IDS_RUN == {81, 82}
