"""ssg_conv2d_f32 (and ssg_conv2d_igemm_f32) against tests/conv_ref.py on every kernel route, forward and input gradient, through the
C-ABI (pkg._lib.ConvDesc, lib.call, lib.stream_ptr()), not through ops.conv2d.  tests/test_conv_ref.py rehearses every gate used here
on the CPU: a float32 emulation of each route passes it at these very cases, and each planted defect fails it.

Every case of conv_ref.CASES
  * packs its weights with the library's own ssg_pack_weights_f32 and ssg_pack_weights_split_bf16x3 and asserts the packed bytes
    equal the layouts restated from include/ssunet_hip.h (conv_ref.pack_f32 / pack_split / pack_split_k32) -- the pack test;
  * asserts the kernel id, pack format, workspace size, statistics rows and LDS-DMA body the library names FOR THE DESCRIPTOR IT
    LAUNCHES against the literals of the case table (so conv_ref.check_coverage is coverage of what ran);
  * runs three classes of data: (a) integer-valued operands, exact; (b) one non-zero input pixel and channel (at every case),
    exact with a power-of-two operand and within the one-product gate at full mantissas; (c) random full-mantissa
    operands within the hard gate, at most 1 % activation ties, and on the `stat` cases an RMS error of at most RMS_MARGIN = 2 x the
    float32 emulation's;
  * where the case asks for statistics rows (bnpart, bwd_x): every row written, the totals within the derived gates of the fp64
    column sums of the fp32 output the kernel wrote.

Memory: `out` is a channel slice of NaN-filled wider rows where ldo > Cout, between poisoned sentinel bands; the workspace is exactly
ssg_conv2d_workspace_bytes long, NaN-filled and banded; so are the bnpart rows and the packs; inputs, residual and bwd_x are channel
slices of NaN-filled rows.  After the run the bands are intact, no NaN is left in the grid's pixels, the pad lanes Cout .. pad4(Cout)
- 1 are 0, pixels outside a parity class's phase and lanes outside the slice are untouched, and two runs give the same bits.

Non-finite operands (one +inf, one NaN, one 3.4e38 in x, then in w) at the smallest shape of ids 40, 41, 42 and 60..64 (ids 50 / 51:
tests/test_conv_dma_split_once_gpu.py::test_nonfinite_operands_take_the_fp32_class): every element has the class of the fp32
reference, finite ones within the hard gate.  Host refusals return their status and leave `out` untouched.

No defect was found: every case passes on every route, and both pack functions write the documented layouts.

Measured on an MI355X, 2026-10-20: in the run of the whole GPU suite none of the file's 142 tests is among the suite's fifteen
slowest (each under 4.6 s); the file alone, one step earlier with class (b) at five of the thirteen large-grid cases only, took 21.7 s,
its slowest case (halo31_c144_34: 127 000 pixels, 144 -> 34 channels, the floor of id 31) 2.7 s.  Per kernel id over
the 122 cases of conv_ref.CASES (test_conv_case): cases / of which `stat`, worst error / hard gate of class (c) (pass: <= 1), over the
`stat` cases the worst RMS error / RMS error of the float32 emulation (pass: <= 2), over all cases the worst error / one-product gate
of class (b) `full` (pass: <= 1), and the worst error / gate of the statistics totals (S1 and S2; the number of cases with rows in
brackets):

    id  0 conv_igemm<128,128>        5 / 1   0.16     0.999   0.949   -
    id  1 conv_igemm<256,64>         4 / 1   0.16     0.995   0.912   -
    id  2 conv_igemm<256,32>         5 / 1   0.12     1       0.875   -
    id 10 thin small-Cout            4 / 2   0.054    1.02    0.948   -          (one of them igemm_thin_shape: conv_igemm<256,32>)
    id 12 thin4 (4-channel input)    3 / 1   0.32     0.893   0.933   -
    id 13 thin4 (Cout <= 8)          3 / 1   0.0014   0.316   0.898   -
    id 14 tiny4                      3 / 1   0.11     1.76    0.524   -
    id 15 thin32                     3 / 0   0.14     -       0.961   -
    id 16 conv1x1_k64                2 / 0   0.097    -       0.305   -
    id 20 conv_igemm_dma<128,128>    4 / 1   0.017    0.994   0.972   0.0024 (1)
    id 21 conv_igemm_dma<256,64>     5 / 1   0.014    0.987   0.951   0.00062 (1)
    id 22 conv_igemm_dma<128,64>     4 / 1   0.099    1.04    0.919   0.0015 (1)
    id 30 conv_igemm_halo<128,128>   2 / 0   0.045    -       0.977   0.00022 (1)
    id 31 conv_igemm_halo<256,64>    2 / 0   0.006    -       0.469   5e-05 (1)
    id 32 conv_igemm_halo<128,64>    8 / 3   0.013    1       0.953   0.0018 (1)  (four of them split-K)
    id 33 halo16<128,128>            4 / 1   0.023    0.999   0.964   0.0017 (1)  (one split-K)
    id 34 halo16<128,64>             5 / 1   0.025    1.01    0.986   0.0011 (1)  (one split-K)
    id 40 halo_x3<128,128>           2 / 0   0.036    -       0.478   8.2e-05 (1)
    id 41 halo_x3<128,64>            4 / 2   0.012    0.422   0.433   0.00099 (1)
    id 42 merged parity              3 / 1   0.022    0.344   0.235   -
    id 50 dma_x3<64>                 5 / 2   0.059    0.422   0.312   0.00011 (1)
    id 51 dma_x3<128>                4 / 1   0.085    0.364   0.412   0.0003 (1)
    id 60 conv_halo_k32<8,128>      11 / 3   0.023    0.485   0.485   0.0034 (5)
    id 61 conv_halo_k32<4,64>       10 / 3   0.017    0.473   0.479   0.0055 (4)
    id 62 conv_halo_k32<16,64>       7 / 2   0.014    0.405   0.431   0.00097 (4)
    id 63 conv_halo_k32<8,16>        5 / 1   0.0041   0.456   0.315   7.4e-05 (1)
    id 64 conv_halo_k32<8,32>        5 / 1   0.0047   0.458   0.363   0.00015 (1)

  Outside the table: test_nonfinite_operands (8 shapes x 2) every class equal, finite elements at most 0.039 of the hard gate, no element
  on the overflow threshold; test_scaled_pack bit-equal to fl(w fl(1 / sigma)).

  On the fp32-MFMA routes the RMS ratio is 1 within a few percent: the matrix instructions add one product at a time, fused, in the K
  order the emulation restates.  The VALU kernels differ: tiny4 (id 14) errs 1.76 x as much as the emulation's fused chain (its
  summation order is its own; the margin holds), the thin kernels (10, 13) a third as much.  On the split routes the emulation adds
  six products per channel one by one and the matrix unit 16 or 32 channels of one product per instruction: the kernels err less
  than half as much.  The hard gate is met with room everywhere (it charges every addition its worst case).  The one-product gate is
  met at up to 0.99 on the fp32 routes -- a product without bias is one rounding, half an ulp, and the gate u32 |p| is half an ulp at
  the top of a binade -- and at 0.24 .. 0.49 of 8 u32 on the split routes, id 40 included.  The statistics totals lie at well under
  a hundredth of their gates (the gates charge every fp32 chain the whole tile's spread).  Class (a) is exact and two runs give the
  same bits at every case.
"""
import ctypes as C_

import numpy as np
import pytest
import torch

import conv_ref as cr
from conv_ref import F32, F64
from test_wgrad_gpu import GUARD, NAN, POISON, SSG_EALIGN, SSG_EINVAL, _Banded, _rows  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def _k32_mode_restored(pkg):
    yield
    pkg._lib.call('ssg_conv_set_k32_mode', 1)


def _dev(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


class _Launch(object):
    """One case's descriptor over device buffers: packs checked against the restated layouts, out / workspace / rows between bands."""

    def __init__(self, lib, dev, c, d, sigma=None):
        self.lib, self.c, self.g, self.dev = lib, c, cr.geom(c), dev
        g = self.g
        self.keep = []
        a = {}
        b1, a['in1'] = _rows(dev, d.x1, c.C1, g.ld1)
        b2, a['in2'] = _rows(dev, d.x2, c.C2, g.ld2) if c.C2 else (None, None)
        self.keep += [b1, b2]
        for name, arr in (('bias', d.bias), ('scale', d.scale), ('shift', d.shift), ('bscale', d.bscale), ('bshift', d.bshift), ('bmean', d.bmean)):
            if arr is not None:
                t = _dev(dev, cr.f32(arr)); self.keep.append(t); a[name] = t.data_ptr()
        if c.res:
            br, a['res'] = _rows(dev, d.res, c.Cout, g.ldr); self.keep.append(br)
        if c.bwd is not None:
            bb, a['bx'] = _rows(dev, d.bx, c.Cout, g.ldr); self.keep.append(bb)
        # the weights: OIHW on the device, packed by the library, compared with the restated layout bit for bit
        w = _dev(dev, cr.f32(d.w)); self.keep.append(w)
        nt = len(g.taps)
        ky = (C_.c_int * nt)(*[t[0] for t in g.taps]); kx = (C_.c_int * nt)(*[t[1] for t in g.taps])
        O, I = d.w.shape[:2]
        self.wpk = _Banded(g.R * g.Kp * 4, dev)
        if sigma is None:
            lib.call('ssg_pack_weights_f32', C_.c_void_p(w.data_ptr()), O, I, c.k, c.k, g.transpose, nt, ky, kx, g.kmode, g.Cin, g.Kp,
                     C_.c_void_p(self.wpk.addr()), lib.stream_ptr())
        else:
            sg = _dev(dev, np.array([sigma], dtype=F32)); self.keep.append(sg)
            lib.call('ssg_pack_weights_scaled_f32', C_.c_void_p(w.data_ptr()), O, I, c.k, c.k, g.transpose, nt, ky, kx, g.kmode, g.Cin,
                     g.Kp, C_.c_void_p(sg.data_ptr()), C_.c_void_p(self.wpk.addr()), lib.stream_ptr())
        self.packed = self.wpk.body().cpu().numpy().reshape(g.R, g.Kp).copy()
        assert self.wpk.intact(), 'sentinel band beside the fp32 pack overwritten'
        a['w'] = self.wpk.addr()
        # out: [N OH OW] rows of ldo floats, the slice 4 floats in where the row is wide enough
        self.off = 4 if g.ldo >= cr.pad4(c.Cout) + 4 else 0
        self.lanes = min(cr.pad4(c.Cout), g.ldo - self.off)
        self.out = _Banded(c.N * g.OH * g.OW * g.ldo * 4, dev)
        a['out'] = self.out.addr() + 4 * self.off
        self.desc = cr.fill_desc(lib.ConvDesc(), c, a)
        self.split = self.part = self.ws = None
        self.plan = cr.plan_queries(lib, c, self.desc, self._split_pack, self._rows_buf, self._ws_buf)

    def _split_pack(self, fmt):
        c, g = self.c, self.g
        nbytes = self.lib.call('ssg_pack_weights_split_bytes', c.Cout, g.Kp, fmt)
        assert nbytes == cr.split_pack_bytes(c.Cout, g.Kp, fmt)
        self.split = _Banded(nbytes, self.dev)
        self.lib.call('ssg_pack_weights_split_bf16x3', C_.c_void_p(self.wpk.addr() + g.row0 * g.Kp * 4), c.Cout, g.Kp, fmt,
                      C_.c_void_p(self.split.addr()), self.lib.stream_ptr())
        self.split_fmt = fmt
        return self.split.addr()

    def _rows_buf(self, rows):
        self.part = _Banded(rows * 2 * self.c.Cout * 8, self.dev)
        self.nrows = rows
        return self.part.addr()

    def _ws_buf(self, nbytes):
        self.ws = _Banded(nbytes, self.dev)
        return self.ws.addr()

    def check_packs(self, d, sigma=None):
        c, g = self.c, self.g
        want = cr.pack_f32(d.w, g.transpose, g.taps, g.kmode, g.Cin, g.Kp, sigma)
        assert cr.same_bits(self.packed, want), 'ssg_pack_weights_f32: %d of %d floats differ from the layout of include/ssunet_hip.h' % (
            int((self.packed.view(np.int32) != want.view(np.int32)).sum()), want.size)
        if self.split is not None:
            rows = want[g.row0:g.row0 + c.Cout]
            exp = cr.pack_split_k32(rows, self.split_fmt) if self.split_fmt >= 1000 else cr.pack_split(rows, self.split_fmt)
            got = self.split.buf[GUARD:GUARD + self.split.n].view(torch.int16).cpu().numpy().view(np.uint16)
            assert self.split.intact(), 'sentinel band beside the split pack overwritten'
            assert np.array_equal(got, exp.reshape(-1)), 'ssg_pack_weights_split_bf16x3 (format %d): %d of %d bf16 values differ' % (
                self.split_fmt, int((got != exp.reshape(-1)).sum()), got.size)

    def status(self):
        fn = self.lib.load().ssg_conv2d_igemm_f32 if self.c.entry == 'igemm' else self.lib.load().ssg_conv2d_f32
        return fn(C_.byref(self.desc), self.lib.stream_ptr())

    def raw(self):
        g = self.g
        return self.out.body().cpu().numpy().reshape(self.c.N, g.OH, g.OW, g.ldo).copy()

    def run(self, ref):
        """Two launches into NaN-filled out, workspace and rows: the same bits, the bands intact, NaN exactly where nothing is to be
        written, zeros in the pad lanes.  Returns (out [N, OH, OW, Cout], rows [rows, 2, Cout] or None)."""
        c, g = self.c, self.g
        runs = []
        for _ in range(2):
            self.out.fill()
            for b in (self.ws, self.part):
                if b is not None:
                    b.fill()
            rc = self.status()
            assert rc == 0, 'status %d: %s' % (rc, self.lib.load().ssg_last_error())
            rows = None
            if self.part is not None:
                rows = self.part.buf[GUARD:GUARD + self.part.n].view(torch.float64).cpu().numpy().reshape(self.nrows, 2, c.Cout).copy()
            runs.append((self.raw(), rows))
        assert self.out.intact(), 'sentinel band beside out overwritten'
        assert self.ws is None or self.ws.intact(), 'sentinel band beside the workspace overwritten'
        assert self.part is None or self.part.intact(), 'sentinel band beside the bnpart rows overwritten'
        assert cr.same_bits(runs[0][0], runs[1][0]), 'two runs differ'
        raw, rows = runs[0]
        if rows is not None:
            assert np.array_equal(rows.view(np.int64), runs[1][1].view(np.int64)), 'two runs differ in the statistics rows'
            assert np.isfinite(rows).all(), 'a statistics row was not written'
        w = ref.written[..., 0]
        sl = raw[..., self.off:self.off + self.lanes]
        assert np.isnan(raw[..., :self.off]).all() and np.isnan(raw[..., self.off + self.lanes:]).all(), 'lanes outside the channel slice written'
        assert np.isnan(sl[~w]).all(), 'pixels outside the launch grid / the parity phase written'
        assert not np.isnan(sl[w][:, :c.Cout]).any() or not np.isfinite(ref.out[ref.written]).all(), 'NaN left in the grid'
        assert (sl[w][:, c.Cout:] == 0).all(), 'pad lanes are not 0'
        return sl[..., :c.Cout], rows


def _launch(pkg, dev, c, d):
    L = _Launch(pkg._lib, dev, c, d)
    cr.check_plan(c, L.plan)
    L.check_packs(d)
    return L


def _report(c, ratios):
    print('RATIO id=%d %-26s %s' % (c.kid, c.name, '  '.join('%s=%.3g' % kv for kv in sorted(ratios.items()))))


def _stats_ratios(c, d, ref, got, rows):
    want = cr.stats_of_output(c, d, got, ref.written)
    gates = cr.bwd_stats_gates(c, d, got, ref.written) if c.bwd is not None else cr.stats_gates(c, d, got)
    tot = rows.sum(axis=0)
    return cr.worst_ratio(tot[0] - want[0], gates[0]), cr.worst_ratio(tot[1] - want[1], gates[1])


# ----------------------------------------------------------------------------- 1. every case, classes (a), (b), (c), the packs, the rows
@pytest.mark.parametrize('c', cr.CASES, ids=lambda c: c.name)
def test_conv_case(pkg, dev, c):
    torch.set_num_threads(16)
    g = cr.geom(c)
    ratios = {}
    wants_rows = c.bnpart or c.bwd is not None
    # (a) integers: exact
    d = cr.int_data(c)
    ref = cr.conv_ref(c, d)
    assert cr.int_class_is_exact(c, ref)
    got, rows = _launch(pkg, dev, c, d).run(ref)
    assert cr.equal_values(got, ref.out, ref.written), 'class (a), kernel id %d: %s' % (c.kid, cr.first_mismatch(got, ref.out, ref.written))
    assert (rows is not None) == bool(wants_rows)
    # (c) full mantissas: the hard gate, the tie cap, the rows, and on the stat cases the RMS gate
    d = cr.rand_data(c)
    ref = cr.conv_ref(c, d)
    got, rows = _launch(pkg, dev, c, d).run(ref)
    ratios['hard'], ties = cr.judge(c, g, ref, got, cr.hard_gate(c, g, ref))
    if c.bwd is not None:
        ties = max(ties, cr.bwd_ties(c, d, ref))
    if wants_rows:
        ratios['s1'], ratios['s2'] = _stats_ratios(c, d, ref, got, rows)
    if c.stat:
        em = cr.emul(c, d)[0][..., :c.Cout]
        ratios['rms'] = cr.rms((got.astype(F64) - ref.out)[ref.written]) / cr.rms((em.astype(F64) - ref.out)[ref.written])
    # (b) one non-zero input pixel and channel, at every case
    for variant in ('xpow2', 'wpow2', 'full'):
        d1 = cr.onehot_data(c, variant)
        ref1 = cr.conv_ref(c, d1)
        assert np.count_nonzero(np.nan_to_num(ref1.acc)) > 0
        got1, _ = _launch(pkg, dev, c, d1).run(ref1)
        if variant == 'full':
            ratios['product'] = cr.judge(c, g, ref1, got1, cr.one_product_gate(c, g, ref1))[0]
        else:
            want = ref1.out.astype(F32).astype(F64)
            assert cr.equal_values(got1, want, ref1.written), 'class (b) %s, kernel id %d: %s' % (
                variant, c.kid, cr.first_mismatch(got1, want, ref1.written))
    _report(c, ratios)
    assert ratios['hard'] <= 1, ratios
    assert ties <= 0.01, ties
    assert ratios.get('product', 0) <= 1, ratios
    assert ratios.get('rms', 0) <= cr.RMS_MARGIN, ratios
    assert ratios.get('s1', 0) <= 1 and ratios.get('s2', 0) <= 1, ratios


def test_case_table_covers_every_route():
    cr.check_coverage()


# ----------------------------------------------------------------------------- 2. the scaled pack (spectral norm)
@pytest.mark.parametrize('sigma', [2.0, 1.7109375])
def test_scaled_pack(pkg, dev, sigma):
    """ssg_pack_weights_scaled_f32: W / sigma in the layout of ssg_pack_weights_f32.  A power-of-two sigma is exact; otherwise every
    weight is fl(w fl(1 / sigma)) -- the restated expression, bit for bit -- which is within 2 u32 of w / sigma."""
    c = cr.case('x3_41_dgrad_slice'); g = cr.geom(c)
    d = cr.rand_data(c)
    L = _Launch(pkg._lib, dev, c, d, sigma=sigma)
    L.check_packs(d, sigma=sigma)
    exact = cr.pack_f32(d.w, g.transpose, g.taps, g.kmode, g.Cin, g.Kp).astype(F64) / sigma
    if sigma == 2.0:
        assert np.array_equal(L.packed.astype(F64), exact)
    assert cr.worst_ratio(L.packed.astype(F64) - exact, 2 * cr.U32 * np.abs(exact)) <= 1
    ref = cr.conv_ref(c, d._replace(w=cr.f32(d.w.astype(F64) / sigma)) if sigma == 2.0 else d._replace(w=_unpack(c, g, L.packed, d.w.shape)))
    got, _ = L.run(ref)
    assert cr.judge(c, g, ref, got, cr.hard_gate(c, g, ref))[0] <= 1


def _unpack(c, g, packed, shape):
    """OIHW weights read back from a kmode-0 transposed pack (the weights the launch multiplies by)."""
    w = np.zeros(shape, dtype=F32)
    nt = len(g.taps)
    cc = np.arange(shape[0])
    for t, (ky, kx, _, _) in enumerate(g.taps):
        w[:, :, ky, kx] = packed[:, (cc // 16) * nt * 16 + t * 16 + cc % 16].T
    return w


# ----------------------------------------------------------------------------- 3. non-finite operands on the split routes
@pytest.mark.parametrize('where', ['x', 'w'])
@pytest.mark.parametrize('name', cr.NONFINITE_CASES)
def test_nonfinite_operands(pkg, dev, name, where):
    torch.set_num_threads(16)
    c = cr.case(name); g = cr.geom(c)
    assert c.kid in cr.SPLIT_IDS
    d = cr.nonfinite_data(c, where)
    ref = cr.conv_ref(c, d, elementwise=True)
    with np.errstate(all='ignore'):
        ref32 = ref.out.astype(F32)                # 3.4e38 x w overflows fp32 where |w| > 1.0008: the class is that of the fp32 result
        gate = cr.hard_gate(c, g, ref)
        # a finite pre-activation within the gate of the fp32 overflow threshold (FLT_MAX + half an ulp) may come out on either side of it
        edge = np.isfinite(ref.pre) & np.isfinite(gate) & (np.abs(np.abs(ref.pre) - cr.FLT_MAX * (1 + 2.0 ** -25)) <= gate)
        gate = np.where(np.isfinite(gate), gate, 0.0)     # a finite result of non-finite terms (ReLU of -inf): exactly the reference's
    want = cr.classes(ref32)
    W = ref.written
    assert (want[W] == 0).any() and (want[W] == 3).any()
    L = _Launch(pkg._lib, dev, c, d)
    cr.check_plan(c, L.plan)
    got, _ = L.run(ref)
    cls = cr.classes(got)
    either = edge & ((cls == 0) | (cls == np.where(ref.pre > 0, 1, 2)))
    bad = np.argwhere(W & (cls != want) & ~either)
    assert not len(bad), 'kernel id %d: %d elements in another class than the reference, first %s: got %r, reference %r' % (
        c.kid, len(bad), tuple(bad[0]), got[tuple(bad[0])], ref.out[tuple(bad[0])])
    fin = W & (want == 0) & (cls == 0)
    r = cr.worst_ratio(got[fin].astype(F64) - ref.out[fin], gate[fin])
    _report(c, {'hard_%s' % where: r, 'edge_%s' % where: int(edge[W].sum()), 'nonfinite_%s' % where: int((want[W] != 0).sum())})
    assert r <= 1


# ----------------------------------------------------------------------------- 4. host refusals: a status, no launch, out untouched
def _refused(L, status):
    L.out.fill()
    rc = L.status()
    torch.cuda.synchronize()
    assert rc == status, 'status %d, expected %d' % (rc, status)
    assert bool(torch.isnan(L.out.body()).all().item()) and L.out.intact(), 'a refused call wrote out'


def test_host_refusals(pkg, dev):
    lib = pkg._lib
    q = lambda name, D: lib.call(name, C_.byref(D))
    one = torch.ones(256, device=dev)
    c = cr.case('halo32_c32_136'); d = cr.int_data(c)
    L = _launch(pkg, dev, c, d)
    L.desc.in_scale = one.data_ptr(); L.desc.in_shift = one.data_ptr(); L.desc.in_act = 1
    assert q('ssg_conv2d_in_affine_ok', L.desc) == 0
    _refused(L, SSG_EINVAL)                                       # in_scale on a route without the fused transform
    L = _launch(pkg, dev, c, d)
    part = torch.zeros(4096, dtype=torch.float64, device=dev)
    L.desc.bwd_x = L.out.addr(); L.desc.bwd_ldx = L.g.ldo; L.desc.bwd_scale = one.data_ptr(); L.desc.bwd_shift = one.data_ptr()
    L.desc.bwd_mean = one.data_ptr(); L.desc.bwd_act = 1; L.desc.bnpart = part.data_ptr()
    assert q('ssg_conv2d_bwd_stats_ok', L.desc) == 0
    _refused(L, SSG_EINVAL)                                       # bwd_x on a route without the backward-statistics epilogue
    c2 = cr.case('reg0_c24_134'); d2 = cr.int_data(c2)
    L = _launch(pkg, dev, c2, d2)
    assert q('ssg_conv2d_bnpart_rows', L.desc) == 0
    L.desc.bnpart = part.data_ptr()
    _refused(L, SSG_EINVAL)                                       # bnpart where ssg_conv2d_bnpart_rows is 0
    c3 = cr.case('parity_c16_64'); d3 = cr.int_data(c3)
    L = _launch(pkg, dev, c3, d3)
    L.desc.Cout = 60                                              # no whole 64-column tile: ssg_conv2d_split_bn != 64
    assert q('ssg_conv2d_split_bn', L.desc) != 64
    _refused(L, SSG_EINVAL)                                       # parity_merge without the merged-parity kernel
    c4 = cr.case('x3_41_c32_64'); d4 = cr.int_data(c4)
    L = _launch(pkg, dev, c4, d4)
    L.desc.w_split = L.desc.w_split + 4
    _refused(L, SSG_EALIGN)                                       # a misaligned w_split
    for off in (-3, 6):
        L = _launch(pkg, dev, c, d)
        L.desc.dx[4] = off
        _refused(L, SSG_EINVAL)                                   # a tap offset outside [-2, 5]
    L = _launch(pkg, dev, c, d)
    L.desc.C1 = c.C1 - 2
    _refused(L, SSG_EINVAL)                                       # C1 % 4 != 0
    L = _launch(pkg, dev, c, d)
    L.desc.GH = L.g.GH + 1
    _refused(L, SSG_EINVAL)                                       # a grid exceeding the output image
    L = _launch(pkg, dev, c, d)                                   # and the untouched descriptor still runs
    ref = cr.conv_ref(c, d)
    got, _ = L.run(ref)
    assert cr.equal_values(got, ref.out, ref.written)
