"""ssg_conv2d_wgrad_bf16x1_f32 (csrc/conv_wgrad_k32_bf16.hip, kernel id 72) against tests/wgrad_x1_ref.py, through the C-ABI.
tests/test_wgrad_x1_ref.py rehearses the gates on the CPU: the float32 emulation passes them at these cases, each planted defect
fails one.

Per case of wgrad_x1_ref.CASES:
  (a) integer operands in [-3, 3]: every product and sum is exact in bf16 and fp32 -> bit equality with fp64;
  (b) one non-zero dout pixel, full-mantissa operands: every element is f32(bf16(x) * bf16(dout)), bit for bit (the product of
      two bf16 values is exact in fp32);
  (c) full-mantissa operands: (P + 2) u32 mag + u32 |ref| against fp64 on the rounded operands, and that plus
      (2^-8 + 2^-18) sum |x| |dout| against fp64 on the operands as given.
Every launch: dw and the workspace NaN-filled between poisoned bands, the workspace exactly the queried size, two runs with the
same bits.  Non-finite x (3.4e38, 3.39e38, +-inf, NaN against zero and non-zero dout): every element has the class the fp32-class
kernel (ssg_conv2d_wgrad_f32, id 60) gives on the same buffers.  Host refusals return a status and launch nothing."""
import ctypes as C_

import numpy as np
import pytest
import torch

import wgrad_ref as wr
import wgrad_x1_ref as xr
from wgrad_ref import F32, F64

pytestmark = pytest.mark.gpu

GUARD = 1024
POISON = 0x5A
NAN = float('nan')
SSG_OK, SSG_EINVAL = 0, -1


class _Banded(object):
    """`nbytes` of device memory, NaN-filled, with a poisoned band of GUARD bytes on each side."""

    def __init__(self, nbytes, dev):
        self.n = int(nbytes)
        assert self.n % 4 == 0
        self.buf = torch.empty(self.n + 2 * GUARD, dtype=torch.uint8, device=dev)
        assert (self.buf.data_ptr() + GUARD) % 16 == 0
        self.buf[:GUARD] = POISON; self.buf[GUARD + self.n:] = POISON
        self.fill()

    def body(self):
        return self.buf[GUARD:GUARD + self.n].view(torch.float32)

    def fill(self):
        self.body().fill_(NAN)

    def addr(self):
        return self.buf.data_ptr() + GUARD

    def intact(self):
        return bool((self.buf[:GUARD] == POISON).all().item() and (self.buf[GUARD + self.n:] == POISON).all().item())


def _rows(dev, data, C, ld):
    """data [..., C] as the channel slice [off, off + C) of NaN-filled rows `ld` wide."""
    rows = int(np.prod(data.shape[:-1]))
    off = 4 if ld >= C + 4 else 0
    buf = torch.full((rows, ld), NAN, dtype=torch.float32, device=dev)
    buf[:, off:off + C] = torch.from_numpy(np.ascontiguousarray(data, dtype=F32).reshape(rows, C)).to(dev)
    assert (buf.data_ptr() + 4 * off) % 16 == 0
    return buf, buf.data_ptr() + 4 * off


class _Launch(object):
    def __init__(self, lib, dev, c, data, entry='ssg_conv2d_wgrad_bf16x1'):
        self.lib, self.c, self.g, self.entry = lib, c, wr.geom(c), entry
        g = self.g
        x1, x2, d, _, _ = data
        b1, a1 = _rows(dev, x1, c.C1, g.ld1)
        b2, a2 = _rows(dev, x2, c.C2, g.ld2) if c.C2 else (None, None)
        bd, ad = _rows(dev, d, c.Cout, g.ldd)
        self.keep = [b1, b2, bd]
        self.dw = _Banded(c.Cout * g.cin_real * c.k * c.k * 4, dev)
        self.desc = wr.fill_desc(lib.WgradDesc(), c, a1, a2, ad, self.dw.addr())
        self.ws_bytes = lib.call(entry + '_workspace_bytes', C_.byref(self.desc))
        self.ws = _Banded(max(self.ws_bytes, 16), dev)
        self.desc.ws = self.ws.addr(); self.desc.ws_bytes = self.ws_bytes

    def status(self):
        return getattr(self.lib.load(), self.entry + '_f32')(C_.byref(self.desc), self.lib.stream_ptr())

    def dw_values(self):
        c, g = self.c, self.g
        return self.dw.body().cpu().numpy().reshape(c.Cout, g.cin_real, c.k, c.k).copy()

    def run(self):
        runs = []
        for _ in range(2):
            self.dw.fill(); self.ws.fill()
            self.lib.call(self.entry + '_f32', C_.byref(self.desc), self.lib.stream_ptr())
            runs.append(self.dw_values())
        assert self.ws.intact(), 'sentinel band beside the workspace overwritten'
        assert self.dw.intact(), 'sentinel band beside dw overwritten'
        assert wr.same_bits(runs[0], runs[1]), 'two runs differ'
        return runs[0]


def _launch(pkg, dev, c, data):
    L = _Launch(pkg._lib, dev, c, data)
    assert pkg._lib.call('ssg_conv2d_wgrad_bf16x1_ok', C_.byref(L.desc)) == 1
    assert pkg._lib.call('ssg_conv2d_wgrad_bf16x1_kernel_id', C_.byref(L.desc)) == xr.KERNEL_ID
    assert L.ws_bytes == xr.workspace_bytes(c), 'the library plans %d workspace bytes, the restated plan %d' % (L.ws_bytes, xr.workspace_bytes(c))
    return L


def test_case_table():
    assert all(xr.ok(c) for c in xr.CASES)
    _, _, _, steps, sps, splits = xr.plan(xr.case(xr.RAGGED))
    assert splits > 1 and steps % sps != 0 and sps % xr.case(xr.RAGGED).H != 0       # a ragged last slab; slabs start inside a strip
    assert {c.N for c in xr.CASES} == {1, 3} and {c.Cout for c in xr.CASES} == {64, 128}
    assert {(c.C1, c.C2) for c in xr.CASES} == {(64, 0), (64, 64), (128, 0)}
    assert {(c.H, c.W) for c in xr.CASES} >= {(3, 17), (5, 33), (9, 40), (2, 64)}


@pytest.mark.parametrize('c', xr.CASES, ids=lambda c: c.name)
def test_wgrad_x1_case(pkg, dev, c):
    g = wr.geom(c)
    # (a) integers in [-3, 3]: exact
    data = wr.int_data(c)
    assert max(float(np.abs(a).max()) for a in data[:3] if a is not None) <= 3
    ref, mag = wr.wgrad_ref(c, *data)
    assert wr.int_class_is_exact(c, mag)
    dw = _launch(pkg, dev, c, data).run()
    assert wr.equal_values(dw, ref), 'integer operands: %s' % wr.first_mismatch(dw, ref)
    # (b) one non-zero dout pixel: each element one exact product of the rounded operands
    data = wr.onehot_data(c, 'full')
    ref1, _ = xr.ref_rounded(c, data)
    dw1 = _launch(pkg, dev, c, data).run()
    assert np.count_nonzero(ref1) > ref1.size // 2
    assert wr.equal_values(dw1, ref1), 'one-hot dout pixel: %s' % wr.first_mismatch(dw1, ref1)
    # (c) full mantissas: both bounds
    data = wr.rand_data(c)
    ref_r, mag_r = xr.ref_rounded(c, data)
    ref_e, mag_e = xr.ref_exact(c, data)
    dw = _launch(pkg, dev, c, data).run()
    r_rounded = wr.worst_ratio(dw.astype(F64) - ref_r, xr.gate_rounded(c, ref_r, mag_r))
    r_exact = wr.worst_ratio(dw.astype(F64) - ref_e, xr.gate_exact(c, ref_r, mag_r, mag_e))
    print('RATIO id=72 %-20s P=%d splits=%d rounded=%.3g exact=%.3g' % (c.name, g.P, xr.plan(c)[5], r_rounded, r_exact))
    assert r_rounded <= 1 and r_exact <= 1, (r_rounded, r_exact)


def test_nonfinite_operands(pkg, dev):
    c = xr.case(xr.NONFINITE_CASE)
    data = xr.nonfinite_data(c)
    L = _launch(pkg, dev, c, data)
    dw = L.run()
    # the fp32-class kernel on the same operands
    L32 = _Launch(pkg._lib, dev, c, data, entry='ssg_conv2d_wgrad')
    assert pkg._lib.call('ssg_conv2d_wgrad_kernel_id', C_.byref(L32.desc)) == 60
    dw32 = L32.run()
    with np.errstate(all='ignore'):
        ref, _ = wr.wgrad_ref(c, *data, elementwise=True)
        want = wr.classes(ref.astype(F32))
    assert (want == 0).any() and (want == 3).any() and (want == 1).any() and (want == 2).any()
    got, got32 = wr.classes(dw), wr.classes(dw32)
    assert np.array_equal(got32, want), 'the fp32-class kernel and the fp64 reference disagree on %d classes' % int((got32 != want).sum())
    bad = np.argwhere(got != got32)
    assert not len(bad), '%d elements in another class than the fp32 kernel, first %s: got %r, fp32 kernel %r' % (
        len(bad), tuple(bad[0]), dw[tuple(bad[0])], dw32[tuple(bad[0])])
    # 3.4e38 against zero dout: finite in fp32 (3.4e38 * 0 = 0), NaN with a bf16 infinity -- the guard's case
    co_all = dw[:, 3]
    assert np.isfinite(co_all).all()


def _refused(lib, L):
    L.dw.fill(); L.ws.fill()
    assert lib.call('ssg_conv2d_wgrad_bf16x1_ok', C_.byref(L.desc)) == 0
    assert lib.call('ssg_conv2d_wgrad_bf16x1_kernel_id', C_.byref(L.desc)) == SSG_EINVAL
    L.desc.ws_bytes = 1 << 30                      # not the workspace check: the shape is what is refused
    rc = L.status()
    torch.cuda.synchronize()
    assert rc == SSG_EINVAL, 'status %d' % rc
    assert bool(torch.isnan(L.dw.body()).all().item()) and L.dw.intact(), 'a refused call wrote dw'
    assert bool(torch.isnan(L.ws.body()).all().item()), 'a refused call wrote the workspace'


def test_host_refusals(pkg, dev):
    lib = pkg._lib
    for c in (wr._c('s2', 1, 8, 40, 64, 0, 64, stride=2), wr._c('k1', 1, 4, 40, 64, 0, 64, k=1),
              wr._c('c32', 1, 4, 40, 32, 0, 64), wr._c('w16', 1, 4, 16, 64, 0, 64)):
        assert not xr.ok(c)
        _refused(lib, _Launch(lib, dev, c, wr.int_data(c)))
    c = xr.case('x1_w17')
    L = _Launch(lib, dev, c, wr.int_data(c))
    sc = torch.ones(c.C1, device=dev); sh = torch.zeros(c.C1, device=dev)
    L.desc.in_scale = sc.data_ptr(); L.desc.in_shift = sh.data_ptr()
    _refused(lib, L)
    L = _launch(pkg, dev, c, wr.int_data(c))
    L.desc.ws_bytes = L.ws_bytes - 1               # workspace one byte short
    L.dw.fill()
    assert L.status() == SSG_EINVAL
    torch.cuda.synchronize()
    assert bool(torch.isnan(L.dw.body()).all().item())
    L = _launch(pkg, dev, c, wr.int_data(c))        # and the untouched descriptor still runs
    ref, _ = wr.wgrad_ref(c, *wr.int_data(c))
    assert wr.equal_values(L.run(), ref)
