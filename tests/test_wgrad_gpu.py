"""ssg_conv2d_wgrad_f32 (and ssg_linear_wgrad_f32) against tests/wgrad_ref.py on every kernel route, through the C-ABI.
tests/test_wgrad_ref.py rehearses every gate used here on the CPU: a float32 emulation of each route passes it at these very
cases, and each planted defect fails it.

Every case of wgrad_ref.CASES asserts the kernel id the library names for the descriptor it actually passes (so
wgrad_ref.check_coverage -- all fourteen reachable ids x the features each route accepts, both wgrad_reduce_kernel instantiations (by the
restated host rule, see below), the three in_act forms of wgrad_k32_kernel<true> -- is coverage of what ran), and runs three classes of data:

  (a) integer-valued operands: the result must equal the fp64 reference exactly, on every route -- the indexing test;
  (b) one non-zero dout pixel (cases marked `stat`; a fused input transform stays on): with dout or x a power of two the result
      must be exact; with both at full mantissa each element is one product, gated at 8 u32 |x d| on the split routes (the
      derivation is beside wgrad_ref.product_gate) and at one rounding on the fp32-MFMA routes;
  (c) random full-mantissa operands: per element (P + c) u32 mag + u32 |ref| (wgrad_ref.hard_gate), and on the `stat` cases the
      RMS error over the tensor against RMS_MARGIN = 2 x the RMS error of the float32 emulation with the same slab partition.

Every output is pre-filled with NaN, the workspace is exactly ssg_conv2d_wgrad_workspace_bytes long and NaN-filled, sentinel
bands on both sides of the workspace and of dw are checked after the run, dw holds Cin_real channels only (a written pad channel
lands on a neighbour or in the band: class (a) or the band shows it), inputs and dout are channel slices of NaN-filled wider
rows where the case says ld > C, and every launch runs twice and must give the same bits.  Non-finite operands (one +inf, one
NaN, one 3.4e38 in x, then in dout) at the smallest k32, halo_x3 and dma_x3 shapes must give every element the class of the
reference.  Host refusals return their status and leave dw untouched.

No defect was found: every case passes on every route.

Measured on an MI355X, 2026-10-19: the file's 89 tests take 6 s in all, the slowest case 0.6 s.  The table counts the 79 cases of
wgrad_ref.CASES only (test_wgrad_case; the three linear_* conv cases are among them, under ids 15, 20 and 50), per kernel id:
cases / of which `stat`, worst error / hard gate of class (c) (pass: <= 1), and over the `stat` cases the worst RMS error / RMS
error of the float32 emulation (pass: <= 2) and the worst error / product gate of class (b) `full` (pass: <= 1):

    id  2 wgrad_kernel<128,32>      7 / 1   0.17      1        0.986
    id 15 wgrad4 thin dout          6 / 1   0.29      1        0.938
    id 16 wgrad4 thin in            6 / 1   0.0026    1        0.986
    id 17 wgrad_tiny4               3 / 1   0.045     1        0.894
    id 18 wgrad32_cin               4 / 1   4.2e-6    1        0.984
    id 20 wgrad_dma<128,128>        6 / 1   0.40      1        0.964
    id 21 wgrad_dma<128,64>         5 / 1   0.13      1        0.983
    id 30 wgrad_halo<32,128>        5 / 1   0.11      1        0.995
    id 31 wgrad_halo<64,64>         5 / 1   0.11      1        0.984
    id 40 wgrad_halo_x3<32,128>     5 / 2   0.19      0.477    0.282
    id 41 wgrad_halo_x3<64,64>      5 / 2   0.054     0.429    0.292
    id 50 wgrad_dma_x3<128,128>     6 / 2   0.16      0.426    0.253
    id 51 wgrad_dma_x3<128,64>      5 / 2   0.048     0.428    0.257
    id 60 wgrad_k32                11 / 4   0.012     0.477    0.281

  Outside the table: test_linear_wgrad (2 shapes) 0.42 of the hard gate for ssg_linear_wgrad_f32 and 0.26 for the same product as
  a conv; test_nonfinite_operands (3 shapes x 2) every class equal, finite elements at most 0.084 of the hard gate, no element
  on the overflow threshold.

  On the fp32 routes (2, 15..18, 20, 21, 30, 31) the RMS ratio is 1 because the kernels return the emulation's bits: the fp32
  matrix instructions (and the VALU kernel) add one pixel's product at a time, fused, in the order the emulation restates.  On
  the split routes the emulation adds six products per pixel one by one, the matrix unit adds 16 or 32 pixels of one product
  per instruction: the kernels err less than half as much.  No route needs more than the 2 x margin.  The hard gate is met with
  room everywhere (it charges every addition its worst case); the one-product gate of class (b) is met at a half ulp on the fp32
  routes (a single rounding) and at 0.29 x 8 u32 on the split routes.  Class (a) is exact and two runs give the same bits at every case.

  Which wgrad_reduce_kernel instantiation a case runs (<8> or <32>) is not observed: the library offers no query for it, so that
  part of the coverage rests on wgrad_ref._zl, a restatement of the host rule; only the slab count it depends on is pinned.
"""
import ctypes as C_

import numpy as np
import pytest
import torch

import wgrad_ref as wr
from wgrad_ref import F32, F64

pytestmark = pytest.mark.gpu

GUARD = 1024                 # bytes of sentinel on each side
POISON = 0x5A
NAN = float('nan')
SSG_OK, SSG_EINVAL, SSG_EALIGN = 0, -1, -2


@pytest.fixture(scope='module', autouse=True)
def _k32_mode_restored(pkg):
    yield
    pkg._lib.call('ssg_wgrad_set_k32_mode', 1)


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
    """data [..., C] as the channel slice [off, off + C) of NaN-filled rows `ld` wide; the pad lanes C .. pad4(C) - 1 hold zeros
    (the NHWC contract).  Returns (tensor kept alive, address of the slice)."""
    rows = int(np.prod(data.shape[:-1]))
    c4 = wr.pad4(C)
    off = 4 if ld >= c4 + 4 else 0
    buf = torch.full((rows, ld), NAN, dtype=torch.float32, device=dev)
    buf[:, off:off + c4] = 0
    buf[:, off:off + C] = torch.from_numpy(np.ascontiguousarray(data, dtype=F32).reshape(rows, C)).to(dev)
    assert (buf.data_ptr() + 4 * off) % 16 == 0
    return buf, buf.data_ptr() + 4 * off


class _Launch(object):
    """One case's descriptor over device buffers: the tensors of `data`, dw and the workspace between sentinel bands."""

    def __init__(self, lib, dev, c, data):
        self.lib, self.c, self.g = lib, c, wr.geom(c)
        g = self.g
        x1, x2, d, sc, sh = data
        lib.call('ssg_wgrad_set_k32_mode', c.k32)
        self.keep = []
        b1, a1 = _rows(dev, x1, c.C1, g.ld1)
        b2, a2 = _rows(dev, x2, c.C2, g.ld2) if c.C2 else (None, None)
        bd, ad = _rows(dev, d, c.Cout, g.ldd)
        self.keep += [b1, b2, bd]
        a_sc = a_sh = None
        if c.aff is not None and sc is not None:
            tsc = torch.from_numpy(wr.f32(sc)).to(dev); tsh = torch.from_numpy(wr.f32(sh)).to(dev)
            self.keep += [tsc, tsh]
            a_sc, a_sh = tsc.data_ptr(), tsh.data_ptr()
        self.dw = _Banded(c.Cout * g.cin_real * c.k * c.k * 4, dev)
        self.desc = wr.fill_desc(lib.WgradDesc(), c, a1, a2, ad, self.dw.addr(), scale=a_sc, shift=a_sh)
        self.ws_bytes = lib.call('ssg_conv2d_wgrad_workspace_bytes', C_.byref(self.desc))
        self.ws = _Banded(self.ws_bytes, dev)
        self.desc.ws = self.ws.addr(); self.desc.ws_bytes = self.ws_bytes

    def kernel_id(self):
        return self.lib.call('ssg_conv2d_wgrad_kernel_id', C_.byref(self.desc))

    def status(self):
        """The raw status of one launch attempt."""
        return self.lib.load().ssg_conv2d_wgrad_f32(C_.byref(self.desc), self.lib.stream_ptr())

    def dw_values(self):
        c, g = self.c, self.g
        return self.dw.body().cpu().numpy().reshape(c.Cout, g.cin_real, c.k, c.k).copy()

    def run(self):
        """Two launches into NaN-filled dw and workspace: the same bits, the bands intact.  Returns dw."""
        runs = []
        for _ in range(2):
            self.dw.fill(); self.ws.fill()
            self.lib.call('ssg_conv2d_wgrad_f32', C_.byref(self.desc), self.lib.stream_ptr())
            runs.append(self.dw_values())
        assert self.ws.intact(), 'sentinel band beside the workspace overwritten'
        assert self.dw.intact(), 'sentinel band beside dw overwritten'
        assert wr.same_bits(runs[0], runs[1]), 'two runs differ'
        return runs[0]


def _launch(pkg, dev, c, data):
    L = _Launch(pkg._lib, dev, c, data)
    p = wr.make_plan(c)
    assert L.kernel_id() == p.kid, 'the library names kernel id %d, the table expects %d' % (L.kernel_id(), p.kid)
    assert L.ws_bytes == wr.workspace_bytes(c)
    return L


def _report(c, kid, ratios):
    print('RATIO id=%d zl=%d %-24s %s' % (kid, wr.make_plan(c).zl, c.name, '  '.join('%s=%.3g' % kv for kv in sorted(ratios.items()))))


# ----------------------------------------------------------------------------- 1. every case, classes (a), (b), (c)
@pytest.mark.parametrize('c', wr.CASES, ids=lambda c: c.name)
def test_wgrad_case(pkg, dev, c):
    g = wr.geom(c); p = wr.make_plan(c)
    split = p.kid in wr.SPLIT_IDS
    ratios = {}
    # (a) integers: exact
    data = wr.int_data(c)
    ref, mag = wr.wgrad_ref(c, *data)
    assert wr.int_class_is_exact(c, mag)
    dw = _launch(pkg, dev, c, data).run()
    assert wr.equal_values(dw, ref), 'class (a), kernel id %d: %s' % (p.kid, wr.first_mismatch(dw, ref))
    # (c) full mantissas: the hard gate, and on the stat cases the RMS gate
    data = wr.rand_data(c)
    ref, mag = wr.wgrad_ref(c, *data)
    dw = _launch(pkg, dev, c, data).run()
    ratios['hard'] = wr.worst_ratio(dw.astype(F64) - ref, wr.hard_gate(ref, mag, g.P, split))
    if c.stat:
        em, _ = wr.emul_dw(c, wr.emul(c, *data))
        ratios['rms'] = wr.rms(dw.astype(F64) - ref) / wr.rms(em.astype(F64) - ref)
    # (b) one non-zero dout pixel
    if c.stat:
        for variant in ('dpow2', 'xpow2', 'full'):
            data = wr.onehot_data(c, variant)
            ref1, _ = wr.wgrad_ref(c, *data)
            dw1 = _launch(pkg, dev, c, data).run()
            if variant == 'full':
                ratios['product'] = wr.worst_ratio(dw1.astype(F64) - ref1, wr.product_gate(ref1, split))
            else:
                assert wr.equal_values(dw1, ref1), 'class (b) %s, kernel id %d: %s' % (variant, p.kid, wr.first_mismatch(dw1, ref1))
    _report(c, p.kid, ratios)
    assert ratios['hard'] <= 1, ratios
    assert ratios.get('product', 0) <= 1, ratios
    assert ratios.get('rms', 0) <= wr.RMS_MARGIN, ratios


def test_case_table_covers_every_route():
    wr.check_coverage()


# ----------------------------------------------------------------------------- 2. the linear layer, both ways, one fp64 product
@pytest.mark.parametrize('nko', wr.LINEAR_CASES, ids=lambda t: '%dx%dx%d' % t)
def test_linear_wgrad(pkg, dev, nko):
    n, k, o = nko
    lib = pkg._lib
    c = wr.case('linear_%d_%d_%d' % nko)
    rng = np.random.RandomState(n * 7 + o)
    ratios = {}
    for cls in ('int', 'full'):
        if cls == 'int':
            x = wr.f32(rng.randint(-8, 9, (n, k))); dy = wr.f32(rng.randint(-8, 9, (n, o)))
        else:
            x = wr._full(rng, (n, k), 0.3); dy = wr._full(rng, (n, o), 0.1)
        ref, mag = wr.linear_ref(x, dy)
        # ssg_linear_wgrad_f32: x rows 8 floats wider than k, dy rows 4 wider than pad4(o)
        bx, ax = _rows(dev, x, k, k + 8)
        bd, ad = _rows(dev, dy, o, wr.pad4(o) + 4)
        out = _Banded(o * k * 4, dev)
        runs = []
        for _ in range(2):
            out.fill()
            lib.call('ssg_linear_wgrad_f32', C_.c_void_p(ax), n, k, k + 8, C_.c_void_p(ad), o, wr.pad4(o) + 4, C_.c_void_p(out.addr()), lib.stream_ptr())
            runs.append(out.body().cpu().numpy().reshape(o, k).copy())
        assert out.intact() and wr.same_bits(runs[0], runs[1])
        # the same gradient as a 1x1 conv on a 1 x n image (ops.py: _Linear.backward when k % 4 != 0 or x is misaligned)
        conv = _launch(pkg, dev, c, (x.reshape(1, 1, n, k), None, dy.reshape(1, 1, n, o), None, None)).run().reshape(o, k)
        if cls == 'int':
            assert wr.equal_values(runs[0], ref), wr.first_mismatch(runs[0], ref)
            assert wr.equal_values(conv, ref), wr.first_mismatch(conv, ref)
        else:
            ratios['linear'] = wr.worst_ratio(runs[0].astype(F64) - ref, wr.hard_gate(ref, mag, n, False))
            ratios['conv'] = wr.worst_ratio(conv.astype(F64) - ref, wr.hard_gate(ref, mag, n, wr.make_plan(c).kid in wr.SPLIT_IDS))
    _report(c, wr.make_plan(c).kid, ratios)
    assert all(v <= 1 for v in ratios.values()), ratios


# ----------------------------------------------------------------------------- 3. non-finite operands on the split routes
@pytest.mark.parametrize('where', ['x', 'dout'])
@pytest.mark.parametrize('name', wr.NONFINITE_CASES)
def test_nonfinite_operands(pkg, dev, name, where):
    c = wr.case(name); g = wr.geom(c); p = wr.make_plan(c)
    assert p.kid in wr.SPLIT_IDS
    data = wr.nonfinite_data(c, where)
    ref, mag = wr.wgrad_ref(c, *data, elementwise=True)
    with np.errstate(all='ignore'):
        ref32 = ref.astype(F32)                  # 3.4e38 x d overflows fp32 where |d| > 1.0008: the class is that of the fp32 result
        gate = wr.hard_gate(ref, mag, g.P, True)
        # a finite reference within the gate of the fp32 overflow threshold (FLT_MAX + half an ulp) may come out on either side of it
        edge = np.isfinite(ref) & (np.abs(np.abs(ref) - wr.FLT_MAX * (1 + 2.0 ** -25)) <= gate)
    want = wr.classes(ref32)
    assert (want == 0).any() and (want == 3).any() and ((want == 1) | (want == 2)).any()
    dw = _launch(pkg, dev, c, data).run()
    got = wr.classes(dw)
    either = edge & ((got == 0) | (got == np.where(ref > 0, 1, 2)))
    bad = np.argwhere((got != want) & ~either)
    assert not len(bad), 'kernel id %d: %d elements in another class than the reference, first %s: got %r, reference %r' % (
        p.kid, len(bad), tuple(bad[0]), dw[tuple(bad[0])], ref[tuple(bad[0])])
    fin = (want == 0) & (got == 0)
    r = wr.worst_ratio(dw[fin].astype(F64) - ref[fin], gate[fin])
    _report(c, p.kid, {'hard_%s' % where: r, 'edge_%s' % where: int(edge.sum())})
    assert r <= 1


# ----------------------------------------------------------------------------- 4. host refusals: a status, no launch, dw untouched
def _refused(L, status):
    L.dw.fill()
    rc = L.status()
    torch.cuda.synchronize()
    assert rc == status, 'status %d, expected %d' % (rc, status)
    assert bool(torch.isnan(L.dw.body()).all().item()) and L.dw.intact(), 'a refused call wrote dw'


def test_host_refusals(pkg, dev):
    c = wr.case('halox3_w15_h2')
    data = wr.int_data(c)
    L = _launch(pkg, dev, c, data)
    L.desc.ws_bytes = L.ws_bytes - 1
    _refused(L, SSG_EINVAL)                                       # workspace one byte short
    L = _launch(pkg, dev, c, data)
    sc = torch.ones(c.C1, device=dev); sh = torch.ones(c.C1, device=dev)
    L.desc.in_scale = sc.data_ptr(); L.desc.in_shift = sh.data_ptr(); L.desc.in_act = 1
    assert pkg._lib.call('ssg_conv2d_wgrad_in_affine_ok', C_.byref(L.desc)) == 0
    _refused(L, SSG_EINVAL)                                       # in_scale on a route without the fused transform
    L = _launch(pkg, dev, c, data)
    L.desc.C1 = c.C1 - 2
    _refused(L, SSG_EINVAL)                                       # C1 % 4 != 0
    L = _launch(pkg, dev, c, data)
    L.desc.in1 = L.desc.in1 + 4
    _refused(L, SSG_EALIGN)                                       # a pointer 4 bytes off 16
    L = _launch(pkg, dev, c, data)
    L.desc.dout = L.desc.dout + 8
    _refused(L, SSG_EALIGN)
    for off in (-3, 6):
        L = _launch(pkg, dev, c, data)
        L.desc.dx[4] = off
        _refused(L, SSG_EINVAL)                                   # a tap offset outside [-2, 5]
    L = _launch(pkg, dev, c, data)                                # and the untouched descriptor still runs
    ref, _ = wr.wgrad_ref(c, *data)
    assert wr.equal_values(L.run(), ref)
