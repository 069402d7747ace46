"""The split-once body of the split (bf16x3) LDS-DMA convolution (csrc/conv_igemm_dma_k32.hip, kernel ids 50 / 51): activations
split into bf16 planes on the way into LDS, 32-channel K-steps on the 16x16x32 MFMA, chosen inside ssg_conv_igemm_dma_x3_launch.

Every case records the descriptor of each launch it makes (a spy around ops._timed_call) and asserts first that the library names
kernel id 50 or 51 for it and that ssg_conv_dma_body reports the split-once body (2) -- a case that ran the older body would prove
nothing.  Then, through the same ops calls as tests/test_split_gpu.py:

  * integer-valued operands (weights in [-2, 2], activations up to 2^17 where the reduction is short: two or three bf16 terms per
    value, every product and partial sum below 2^23): the result equals the fp64 reference exactly;
  * N(0,1) operands: max and RMS error against the fp64 reference at most 2 x the error of the fp32-MFMA kernel (SSG_MFMA_SPLIT=0
    through the same call) plus the 1e-6 / 1e-8 floors -- the rule of tests/test_split_gpu.py;
  * two runs give the same bits.

The shapes are the smallest at which each mechanism can go wrong (the family needs N * GH * GW >= 4096, Cout % 64 == 0,
Cin % 16 == 0):

  1x1_32_64        one K-step, BN = 64, 52 = 3 * 16 + 4: a partial tile in x
  1x1_48_128       three 16-channel chunks: the last 32-channel step is half empty; BN = 128; 60 = 3 * 16 + 12
  1x1_48_128_brr   the same with bias + residual + ReLU;  1x1_48_128_lrelu: bias + leaky ReLU (slope 0.25: exact on integers)
  cat_48_80_192    C1 = 48: the second 32-channel chunk straddles both inputs; three 64-column tiles
  dgrad_slice      input gradient of a 1x1 conv with 256 input channels, channel slice [64, 192): row0 into the pack
  s2_64_64         3x3 stride 2 pad 1, 132 x 126 -> 66 x 63: stride-2 taps off the borders, odd output width
  s2_96_128        3x3 stride 2 pad 1, 96 channels: 3 chunks x 9 taps = 27 32-channel steps, an odd count (stage parity of the ring)
  classes          the four per-class launches of a stride-2 input gradient (1 / 2 / 2 / 4 taps, output stride 2 with offsets) on a
                   131 x 127 input; class (1, 1) has 65 x 63 = 4095 pixels, below the family's 4096: the fp32 LDS-DMA kernel runs it

Short-K runs (several pixel tiles per workgroup) are not part of the body, so there is no run-edge case.

Measured on an MI355X: the file takes 2.7 s; max error 0.32-1.0 x and RMS error 0.36-0.91 x the fp32-MFMA kernel's (gate: 2).
"""
import ctypes as C_

import pytest
import torch
import torch.nn.functional as F

from test_split_gpu import _run, _same_class

pytestmark = pytest.mark.gpu


class _Spy(object):
    """Records (kernel id, ssg_conv_dma_body) of every conv launch made through ops while active."""

    def __init__(self, pkg):
        self.pkg, self.ops, self.seen = pkg, pkg.ops, []
        fn = pkg._lib.load().ssg_conv_dma_body
        fn.argtypes = [C_.POINTER(pkg._lib.ConvDesc)]
        fn.restype = C_.c_int
        self.body = fn

    def __enter__(self):
        self.orig = self.ops._timed_call

        def spy(kind, entry, d, *a, **k):
            if entry == 'ssg_conv2d_f32':
                self.seen.append((self.pkg._lib.call('ssg_conv2d_kernel_id', C_.byref(d)), self.body(C_.byref(d))))
            return self.orig(kind, entry, d, *a, **k)
        self.ops._timed_call = spy
        return self

    def __exit__(self, *a):
        self.ops._timed_call = self.orig


def _split_once(pkg, fn, want=None):
    """fn() with the split kernels on; every launch must be (id 50 / 51, body 2), or `want(seen)` judges the list."""
    with _Spy(pkg) as spy:
        y = _run(pkg.ops, True, fn)
    assert spy.seen, 'no conv launch was made'
    if want is None:
        assert all(i in (50, 51) and b == 2 for i, b in spy.seen), 'not the split-once body: (kernel id, body) = %s' % spy.seen
    else:
        want(spy.seen)
    return y


class Case(object):
    def __init__(self, name, x_shape, w_shape, K, build, ref, want=None, extra=()):
        self.name, self.x_shape, self.w_shape, self.K, self.build, self.ref, self.want, self.extra = name, x_shape, w_shape, K, build, ref, want, extra


def _fwd(stride, pad, c1=None, bias=False, res=False, act=0, slope=0.0):
    def build(ops, dev, xc, wc, ex):
        x1 = ops.to_nhwc((xc if c1 is None else xc[:, :c1]).to(dev))
        x2 = None if c1 is None else ops.to_nhwc(xc[:, c1:].to(dev))
        w = wc.to(dev)
        b = ex[0].to(dev) if bias else None
        r = ops.to_nhwc(ex[1].to(dev)) if res else None
        return lambda: ops._conv_fwd_impl(x1, x2, w, b, stride, pad, act, slope, res=r)

    def ref(xc, wc, ex):
        y = F.conv2d(xc.double(), wc.double(), ex[0].double() if bias else None, stride, pad)
        if res:
            y = y + ex[1].double()
        return F.relu(y) if act == 1 else F.leaky_relu(y, slope) if act == 2 else y
    return build, ref


def _dgrad(stride, pad, h, w, c_lo, c_hi, merge=True):
    def build(ops, dev, dyc, wc, ex):
        dy = ops.to_nhwc(dyc.to(dev)); wd = wc.to(dev)

        def fn():
            saved = ops.PARITY_MERGE
            ops.PARITY_MERGE = merge
            try:
                return ops._conv_dgrad_impl(dy, wd, stride, pad, h, w, c_lo, c_hi)
            finally:
                ops.PARITY_MERGE = saved
        return fn

    def ref(dyc, wc, ex):
        return torch.nn.grad.conv2d_input((dyc.shape[0], wc.shape[1], h, w), wc.double(), dyc.double(), stride, pad)[:, c_lo:c_hi]
    return build, ref


def _classes_want(seen):
    # classes (0,0), (0,1), (1,0): 66x64, 66x63, 65x64 pixels -> the family, split-once body; (1,1): 65 x 63 = 4095 < 4096 -> not the family
    assert len(seen) == 4, seen
    assert all(i == 50 and b == 2 for i, b in seen[:3]), seen
    assert seen[3][0] not in (50, 51) and seen[3][1] != 2, seen


ACT_RELU, ACT_LRELU = 1, 2
CASES = [
    Case('1x1_32_64', (2, 32, 40, 52), (64, 32, 1, 1), 32, *_fwd(1, 0)),
    Case('1x1_48_128', (1, 48, 72, 60), (128, 48, 1, 1), 48, *_fwd(1, 0)),
    Case('1x1_48_128_brr', (1, 48, 72, 60), (128, 48, 1, 1), 48, *_fwd(1, 0, bias=True, res=True, act=ACT_RELU), extra=((128,), (1, 128, 72, 60))),
    Case('1x1_48_128_lrelu', (1, 48, 72, 60), (128, 48, 1, 1), 48, *_fwd(1, 0, bias=True, act=ACT_LRELU, slope=0.25), extra=((128,),)),
    Case('cat_48_80_192', (1, 128, 72, 60), (192, 128, 1, 1), 128, *_fwd(1, 0, c1=48)),
    Case('dgrad_slice', (1, 128, 72, 60), (128, 256, 1, 1), 128, *_dgrad(1, 0, 72, 60, 64, 192)),
    Case('s2_64_64', (1, 64, 132, 126), (64, 64, 3, 3), 576, *_fwd(2, 1)),
    Case('s2_96_128', (2, 96, 92, 92), (128, 96, 3, 3), 864, *_fwd(2, 1)),
    Case('classes', (1, 64, 66, 64), (64, 64, 3, 3), 256, *_dgrad(2, 1, 131, 127, 0, 64, merge=False), want=_classes_want),
]
EXPECT_ID = {'1x1_32_64': 50, '1x1_48_128': 51, '1x1_48_128_brr': 51, '1x1_48_128_lrelu': 51, 'cat_48_80_192': 50, 'dgrad_slice': 51,
             's2_64_64': 50, 's2_96_128': 51}


def _ints(shape, bound, g):
    return torch.randint(-bound, bound + 1, shape, generator=g).float()


@pytest.mark.parametrize('c', CASES, ids=lambda c: c.name)
def test_split_once_case(pkg, dev, c):
    ops = pkg.ops
    torch.set_num_threads(16)
    g = torch.Generator().manual_seed(101)

    def ids_ok(seen):
        assert all(b == 2 for _, b in seen) and all(i == EXPECT_ID[c.name] for i, _ in seen), (c.name, seen)
    want = c.want or ids_ok

    # integers: |w| <= 2, |x| <= B with 2 * B * K < 2^23 (B <= 2^17: up to three bf16 terms per activation); bias / residual integers
    B = min(1 << 17, (1 << 22) // (2 * c.K))
    xi, wi = _ints(c.x_shape, B, g), _ints(c.w_shape, 2, g)
    exi = tuple(_ints(s, 1000, g) for s in c.extra)
    fn = c.build(ops, dev, xi, wi, exi)
    y = _split_once(pkg, fn, want).cpu().double()
    ref = c.ref(xi, wi, exi)
    assert ref.abs().max().item() < 2 ** 24
    assert torch.equal(y, ref), 'integers: %d of %d elements differ, worst %.3g' % (int((y != ref).sum()), ref.numel(), (y - ref).abs().max().item())

    # N(0,1): the error of the fp32-MFMA kernel through the same call is the yardstick
    xr, wr_ = torch.randn(c.x_shape, generator=g), torch.randn(c.w_shape, generator=g)
    exr = tuple(torch.randn(s, generator=g) for s in c.extra)
    fn = c.build(ops, dev, xr, wr_, exr)
    y3 = _split_once(pkg, fn, want)
    y3b = _split_once(pkg, fn, want)
    assert torch.equal(y3, y3b), 'two runs differ in %d elements' % int((y3 != y3b).sum())
    y32 = _run(ops, False, fn).cpu().double()
    ref = c.ref(xr, wr_, exr)
    e3, e32 = (y3.cpu().double() - ref).abs(), (y32 - ref).abs()
    m3, m32 = e3.max().item(), e32.max().item()
    r3, r32 = e3.pow(2).mean().sqrt().item(), e32.pow(2).mean().sqrt().item()
    print('RATIO %-18s max split=%.3g fp32=%.3g  rms split=%.3g fp32=%.3g' % (c.name, m3, m32, r3, r32))
    assert m3 <= 2.0 * m32 + 1e-6, (m3, m32)
    assert r3 <= 2.0 * r32 + 1e-8, (r3, r32)


@pytest.mark.parametrize('cout', [128, 256])
def test_partial_rows_are_the_column_sums_of_the_output(pkg, dev, cout):
    """want_bn at the 1x1 48 -> 128 shape (36 tiles of 8 x 16, the last column of tiles partly outside the image) and at 48 -> 256 (two
    column tiles: the n0 offset of the partial row and of the wave's columns): the rows summed are the column sums of what the
    kernel wrote, at the tolerances of tests/test_split_gpu.py."""
    ops = pkg.ops
    g = torch.Generator().manual_seed(103)
    xc = torch.randn((1, 48, 72, 60), generator=g) * 1.5 + 0.3
    wc = torch.randn((cout, 48, 1, 1), generator=g) / 48 ** 0.5
    x = ops.to_nhwc(xc.to(dev)); w = wc.to(dev)

    def ok(seen):
        assert seen == [(51, 2)], seen
    yb, pb = _split_once(pkg, lambda: ops._conv_fwd_impl(x, None, w, None, 1, 0, 0, 0.0, want_bn=True), ok)
    assert pb is not None and tuple(pb.shape) == (9 * 4, 2, cout)
    yd = yb.double()
    s1 = yd.sum((0, 2, 3)); s2 = (yd * yd).sum((0, 2, 3))
    tot = pb.sum(0)
    assert torch.allclose(tot[0], s1, rtol=1e-7, atol=1e-6 * yd.abs().sum((0, 2, 3)).max().item())
    assert torch.allclose(tot[1], s2, rtol=1e-6)
    ref = F.conv2d(xc.double(), wc.double())
    assert (yb.cpu().double() - ref).abs().max().item() < 1e-4


@pytest.mark.parametrize('name', ['1x1_32_64', 's2_64_64'])
def test_nonfinite_operands_take_the_fp32_class(pkg, dev, name):
    """One +Inf, one -Inf and one NaN activation, then one NaN weight: every output element is of the fp32-MFMA kernel's class
    (finite / +inf / -inf / NaN) and the finite ones agree within the bounds of tests/test_split_gpu.py::_same_class."""
    ops = pkg.ops
    c = [k for k in CASES if k.name == name][0]
    g = torch.Generator().manual_seed(107)
    xc = torch.randn(c.x_shape, generator=g) * 1.5 + 0.3
    wc = torch.randn(c.w_shape, generator=g) / c.K ** 0.5
    xb = xc.clone()
    n, ci, h, w = c.x_shape
    for v, (ch, yy, xx) in zip((float('inf'), float('-inf'), float('nan')), ((3, 5, 7), (ci - 2, h // 2 + 1, w - 1), (ci // 2, h - 1, 0))):
        xb[n - 1, ch, yy, xx] = v
    wb = wc.clone()
    wb[c.w_shape[0] - 3, ci // 2 + 1, c.w_shape[2] - 1, 0] = float('nan')

    def ok(seen):
        assert seen == [(EXPECT_ID[name], 2)], seen
    for what, xs, ws in (('special activations', xb, wc), ('NaN weight', xc, wb)):
        fn = c.build(ops, dev, xs, ws, ())
        want = _run(ops, False, fn)
        got = _split_once(pkg, fn, ok)
        _same_class(got, want, '%s, %s' % (name, what))
