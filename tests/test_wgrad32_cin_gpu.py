"""wgrad32_cin_kernel (kernel id 18: in has 4 channels, 3x3, Cout >= 32 on >= 65536 pixels) after the one-fragment rewrite, through
the C-ABI with the launcher of tests/test_wgrad_gpu.py: dw and the workspace NaN-filled between sentinel bands, the workspace
exactly ssg_conv2d_wgrad_workspace_bytes long, every launch twice with equal bits, id 18 asserted at every case.

The kernel has two bodies, chosen by Cin_real:
  3  the B columns are n = tap * 3 + c (27 of 32): the pad lane of x is never read and its slab rows stay unwritten (the
     reducer drops them);
  4  taps 0..7 fill the 32 columns, tap 8 runs on the 4x4x1 MFMA with the even and the odd pixels of a pair in two accumulators
     that are added at the fold.
Each at Cout 64 (one channel group), 128 (two) and 96 (a half-empty second group), on N = 2, H = 182, W = 181 (the last 32-pixel
segment of a row holds 21 pixels: one full 16-pixel step and a 5-pixel one with a half-empty last pair; both image borders) and on
N = 1, H = W = 256; the Cout-96 cases read dout and x as channel slices of wider NaN-filled rows.

Gates, all from wgrad_ref: class (a) integer operands exact; class (c) full-mantissa operands within hard_gate per element and an
RMS error of at most RMS_MARGIN x that of the float32 emulation with the route's slab partition.  The emulation adds one pixel
at a time per column; so does the kernel except in tap 8 of the Cin_real == 4 body (even pixels + odd pixels), which is why the
RMS gate and not bit equality is the check there.  test_emulation_passes_every_gate rehearses the gates on the CPU at every case.

Besides: Cin_real == 3 with a non-zero value in the pad lane of x (class (a): a multiplied pad lane would land in a real
column of the packed fragment), and for Cin_real == 4 one non-zero dout pixel at the bottom-right corner (tap 8 reads outside
the image: exact zeros) and at the top-left corner (tap 8 reads pixel (1, 1)): each element one product, one rounding.

Measured on an MI355X, 2026-10-21: every case passes; the Cin_real == 3 cases return the emulation's bits (RMS ratio 1), the
Cin_real == 4 cases 0.997-1.000 of its RMS error, the worst element 5.7e-6 of the hard gate, the corner products 0.96 and 0.995 of one
rounding.  The GPU cases take 0.3 s each; the references and the emulation are computed once per case (1-2 s on the CPU) and
shared between the rehearsal and the GPU test.
"""
import numpy as np
import pytest

import wgrad_ref as wr
from wgrad_ref import F32, F64
from test_wgrad_gpu import _launch

ODD = (2, 182, 181)
SQ = (1, 256, 256)


def _case(cr, cout, nhw, ld=False):
    n, h, w = nhw
    name = 'w32cin_r%d_c%d_%dx%dx%d%s' % (cr, cout, n, h, w, '_ld' if ld else '')
    return wr._c(name, n, h, w, 4, 0, cout, cin_real=cr, irange=4, stat=True, ld1=8 if ld else None, ldd=cout + 4 if ld else None)


CASES = [_case(cr, cout, nhw, ld) for cr in (3, 4) for (cout, nhw, ld) in ((64, ODD if cr == 3 else SQ, False), (128, SQ if cr == 3 else ODD, False), (96, ODD, True))]
_memo = {}


def _int_facts(c):
    """Per case, once: the integer data and its reference."""
    if ('int', c.name) not in _memo:
        di = wr.int_data(c)
        ri, mi = wr.wgrad_ref(c, *di)
        assert wr.int_class_is_exact(c, mi)
        _memo['int', c.name] = (di, ri)
    return _memo['int', c.name]


def _facts(c):
    """Per case, once: the integer class, the random data with its reference, gate and the emulation with its RMS error."""
    if c.name not in _memo:
        g = wr.geom(c)
        di, ri = _int_facts(c)
        dr = wr.rand_data(c)
        rr, mr = wr.wgrad_ref(c, *dr)
        em, guard = wr.emul_dw(c, wr.emul(c, *dr))
        assert guard
        _memo[c.name] = dict(int=di, int_ref=ri, rand=dr, rand_ref=rr, gate=wr.hard_gate(rr, mr, g.P, False), emul=em,
                             emul_rms=wr.rms(em.astype(F64) - rr))
    return _memo[c.name]


def _corner_data(c, corner):
    """Full-mantissa x and one non-zero dout pixel: the first pixel of the tensor or the last."""
    rng = np.random.RandomState(wr._seed(c, 2) + (corner == 'last'))
    x = wr._full(rng, (c.N, c.H, c.W, c.C1), 0.3)
    d = np.zeros((c.N, c.H, c.W, c.Cout), dtype=F32)
    d[(0, 0, 0) if corner == 'first' else (c.N - 1, c.H - 1, c.W - 1)] = wr._full(rng, (c.Cout,), 0.1)
    return x, None, d, None, None


def test_case_list_reaches_the_kernel():
    for c in CASES:
        p = wr.make_plan(c); g = wr.geom(c)
        assert p.kid == 18 and g.P >= 65536 and g.cin_real in (3, 4), c.name
    assert {wr.geom(c).cin_real for c in CASES} == {3, 4}
    assert {c.Cout for c in CASES} == {64, 96, 128}
    assert any(c.W % wr.SEG % 16 and c.W % 2 for c in CASES) and any(wr.geom(c).ldd > wr.pad4(c.Cout) for c in CASES)


@pytest.mark.parametrize('c', CASES, ids=lambda c: c.name)
def test_emulation_passes_every_gate(c):
    f = _facts(c)
    di = f['int']
    em, _ = wr.emul_dw(c, wr.emul(c, *di))
    assert wr.equal_values(em, f['int_ref']), wr.first_mismatch(em, f['int_ref'])
    r = wr.worst_ratio(f['emul'].astype(F64) - f['rand_ref'], f['gate'])
    print('EMUL %-28s hard %.3g  rms %.3g' % (c.name, r, f['emul_rms']))
    assert r <= 1 and f['emul_rms'] > 0


@pytest.mark.gpu
@pytest.mark.parametrize('c', CASES, ids=lambda c: c.name)
def test_wgrad32_cin_case(pkg, dev, c):
    f = _facts(c)
    L = _launch(pkg, dev, c, f['int'])
    assert L.kernel_id() == 18
    dw = L.run()
    assert wr.equal_values(dw, f['int_ref']), 'class (a): %s' % wr.first_mismatch(dw, f['int_ref'])
    L = _launch(pkg, dev, c, f['rand'])
    assert L.kernel_id() == 18
    dw = L.run()
    err = dw.astype(F64) - f['rand_ref']
    hard = wr.worst_ratio(err, f['gate']); rms = wr.rms(err) / f['emul_rms']
    print('RATIO id=18 %-28s hard=%.3g rms=%.3g bits_equal_emul=%s' % (c.name, hard, rms, wr.same_bits(dw, f['emul'])))
    assert hard <= 1
    assert rms <= wr.RMS_MARGIN


@pytest.mark.gpu
def test_pad_lane_of_x_is_never_multiplied(pkg, dev):
    """Cin_real == 3, class (a), x rows 8 wide with 9.0 in the pad lane (channel 3) of every pixel."""
    c = _case(3, 64, SQ, ld=True)
    di, ref = _int_facts(c)
    L = _launch(pkg, dev, c, di)
    assert L.kernel_id() == 18 and wr.geom(c).ld1 == 8
    rows = L.keep[0]                                 # [pixels, 8]: the slice starts at lane 4, the pad lane is lane 7
    assert bool((rows[:, 4:7].cpu().numpy().reshape(c.N, c.H, c.W, 3) == di[0][..., :3]).all())
    rows[:, 7] = 9.0
    dw = L.run()
    assert wr.equal_values(dw, ref), wr.first_mismatch(dw, ref)


@pytest.mark.gpu
@pytest.mark.parametrize('corner', ['first', 'last'])
def test_tap8_at_the_corners(pkg, dev, corner):
    """Cin_real == 4: each dw element is one product of the corner pixel's dout, or an exact zero where the tap leaves the image."""
    c = _case(4, 64, ODD)
    data = _corner_data(c, corner)
    ref, _ = wr.wgrad_ref(c, *data)
    inside = ref[0, 0] != 0                          # [ky, kx]
    want = np.zeros((3, 3), dtype=bool)
    want[1:, 1:] = True
    assert (inside == (want if corner == 'first' else want[::-1, ::-1])).all()
    L = _launch(pkg, dev, c, data)
    assert L.kernel_id() == 18
    dw = L.run()
    r = wr.worst_ratio(dw.astype(F64) - ref, wr.product_gate(ref, False))
    print('RATIO id=18 corner %-5s product=%.3g' % (corner, r))
    assert r <= 1
