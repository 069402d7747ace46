"""The split-once body of the split (bf16x3) LDS-DMA weight gradient (csrc/conv_wgrad_dma_k32.hip, kernel ids 50 / 51): operands
split into bf16 planes on the way into LDS, 32-pixel K-steps on the 16x16x32 MFMA, chosen inside ssg_wgrad_dma_launch.

Every case asserts first that the library names kernel id 50 or 51 for the descriptor it passes and that ssg_wgrad_dma_body
reports the split-once body (2) for it -- a case that ran the older body would prove nothing -- and then checks, through the C-ABI
with the buffers of tests/test_wgrad_gpu.py (NaN-filled dw and workspace between sentinel bands, channel slices of NaN-filled
wider rows where ld > C):

  * integer-valued operands: dw equals the fp64 reference exactly (indexing: taps, strides, borders, tails, masks);
  * full-mantissa operands: every element within wgrad_ref.hard_gate (the bound tests/test_wgrad_gpu.py applies to ids 50 / 51);
  * the RMS error against fp64 at most 2 x that of the fp32-MFMA kernel (flags = 0: ids 20 / 21) on the same buffers, the margin
    tests/test_split_gpu.py uses for the split kernels;
  * two runs give the same bits (the slab reduce is ordered).

The cases are the smallest at which each part of the body can go wrong:

  tail_1x1          Ptot = 189 is no multiple of 16 or 32; steps straddle rows and images (GW = 9); id 51 (BN = 64)
  odd_slices        three K-slices of 17 sixteen-pixel units: every slice ends in a half-empty 32-pixel step whose second half is
                    the next slice's first pixels, and slices 1 and 2 start in the middle of an image row
  s2_odd            3x3 stride 2 pad 1 on 13 x 19 -> 7 x 10: taps off all four borders, odd sizes; id 51
  m216_c96 .. m72_c64   row blocks that straddle taps, M = 216 and 72 (rows >= M masked), Cout 96 (column tail inside a BN = 128
                    tile) and 64
  cat_64_32, cat_8_16   row blocks straddling the two inputs of a concat, ld1 / ld2 wider than C1 / C2, dout a channel slice
                    (ldd > Cout), everything around the slices NaN

Non-finite operands on this label are covered by tests/test_split_gpu.py and tests/test_wgrad_gpu.py (dmax3_1x1_c33), which now run
this body.  Measured on an MI355X: the file takes 2.3 s; worst error / hard gate 0.022, RMS error 0.75-0.85 of the fp32-MFMA
kernel's (gate: 2).
"""
import ctypes as C_

import numpy as np
import pytest

import wgrad_ref as wr
from wgrad_ref import F64
from test_wgrad_gpu import _launch

CASES = [
    wr._c('tail_1x1', 3, 7, 9, 64, 0, 64, k=1),
    wr._c('odd_slices', 2, 20, 20, 8, 0, 256),
    wr._c('odd_slices_12x20', 2, 12, 20, 8, 0, 256),
    wr._c('s2_odd', 2, 13, 19, 64, 0, 64, stride=2),
    wr._c('m216_c96', 2, 9, 11, 24, 0, 96),
    wr._c('m216_c64', 2, 9, 11, 24, 0, 64),
    wr._c('m72_c96', 2, 9, 11, 8, 0, 96),
    wr._c('m72_c64', 2, 9, 11, 8, 0, 64),
    wr._c('cat_64_32', 2, 9, 11, 64, 32, 64, ld1=72, ld2=40, ldd=72),
    wr._c('cat_8_16', 2, 9, 11, 8, 16, 96, ld1=12, ld2=24, ldd=104),
]
EXPECT_ID = {'tail_1x1': 51, 'odd_slices': 50, 'odd_slices_12x20': 50, 's2_odd': 51, 'm216_c96': 50, 'm216_c64': 51, 'm72_c96': 50,
             'm72_c64': 51, 'cat_64_32': 51, 'cat_8_16': 50}


def _body(pkg, L):
    fn = pkg._lib.load().ssg_wgrad_dma_body
    fn.argtypes = [C_.POINTER(pkg._lib.WgradDesc)]
    fn.restype = C_.c_int
    return fn(C_.byref(L.desc))


def _split_once(pkg, dev, c, data):
    L = _launch(pkg, dev, c, data)                        # asserts the kernel id and the workspace size of wgrad_ref.make_plan
    assert L.kernel_id() == EXPECT_ID[c.name]
    assert _body(pkg, L) == 2, 'ssg_wgrad_dma_body reports %d: the split-once body did not take this descriptor' % _body(pkg, L)
    return L


def test_cases_are_what_they_claim():
    p = wr.make_plan(wr._c('odd_slices', 2, 20, 20, 8, 0, 256))
    assert p.kind == 'flat' and p.splits == 3 and p.sps == 17          # an odd number of 16-pixel units per slice
    for c in CASES:
        p = wr.make_plan(c); g = wr.geom(c)
        assert p.kind == 'flat' and p.kid == EXPECT_ID[c.name], (c.name, p)
    g = wr.geom(CASES[0])
    assert g.P == 189 and g.P % 16 and g.GW < 32
    assert (wr.geom(CASES[3]).GH, wr.geom(CASES[3]).GW) == (7, 10)


@pytest.mark.gpu
@pytest.mark.parametrize('c', CASES, ids=lambda c: c.name)
def test_split_once_case(pkg, dev, c):
    g = wr.geom(c)
    # integers: exact
    data = wr.int_data(c)
    ref, mag = wr.wgrad_ref(c, *data)
    assert wr.int_class_is_exact(c, mag)
    dw = _split_once(pkg, dev, c, data).run()             # run(): two launches, the same bits, the bands intact
    assert wr.equal_values(dw, ref), 'integers, kernel id %d: %s' % (EXPECT_ID[c.name], wr.first_mismatch(dw, ref))
    # full mantissas: the hard gate, and the RMS error beside the fp32-MFMA kernel's on the same inputs
    data = wr.rand_data(c)
    ref, mag = wr.wgrad_ref(c, *data)
    dw = _split_once(pkg, dev, c, data).run()
    c32 = c._replace(flags=0)
    L32 = _launch(pkg, dev, c32, data)
    assert L32.kernel_id() == EXPECT_ID[c.name] - 30
    dw32 = L32.run()
    hard = wr.worst_ratio(dw.astype(F64) - ref, wr.hard_gate(ref, mag, g.P, True))
    rms3, rms32 = wr.rms(dw.astype(F64) - ref), wr.rms(dw32.astype(F64) - ref)
    print('RATIO id=%d %-18s hard=%.3g rms_split=%.3g rms_fp32=%.3g' % (EXPECT_ID[c.name], c.name, hard, rms3, rms32))
    assert hard <= 1, hard
    assert rms3 <= 2.0 * rms32 + 1e-8, (rms3, rms32)
