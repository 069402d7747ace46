"""The wide-input -> <= 8-channel 3x3 convolution (`thin4_cout_kernel`, csrc/conv_thin4.hip) in its taps-as-MFMA-rows form, and the
weight gradient of the same layers, against fp64 on the CPU.

Forward: ops.conv2d of a Cin -> Cout layer (Cin 64 / 128, Cout 3 / 4 / 8).  Input gradient: the backward pass of a Cout -> Cin
layer, which launches the same kernel with the transposed weights.  Weight gradient: the backward pass of the forward case.

Bounds: the ones tests/test_ops_gpu.py (test_conv2d_specialised_kernels) applies to these kernels, with the same 1 / sqrt(fan-in)
weights: (rtol 1e-5, atol 2e-6 * sqrt(reduction length)) for the two convolutions, (2e-5, 2e-6 * sqrt(N * H * W)) for the weight
gradient.  Every case prints its max-abs error before it asserts (pytest -s).

Shapes: batch 2 (an image boundary inside the pixel axis); 5 x 7 (narrower than a strip, fewer rows than the LDS ring), 9 x 66 (one
62-pixel strip plus a remainder), 33 x 130 (three strips, two row bands)."""
import math

import pytest
import torch
import torch.nn.functional as F

import layout_probe as lp

pytestmark = pytest.mark.gpu

SIZES = [(5, 7), (9, 66), (33, 130)]
CHANNELS = [(cin, cout) for cin in (64, 128) for cout in (3, 4, 8)]
LABEL = 'thin4_cout_kernel'


def _close(a, b, rtol, atol, what):
    a = a.detach().double().cpu(); b = b.detach().double().cpu()
    err = (a - b).abs()
    print('%s: max abs err %.3e (bound at 0: %.3e)' % (what, err.max().item(), atol))
    bad = err > atol + rtol * b.abs()
    assert not bad.any(), '%s: %d of %d outside the bound, max abs err %.3e' % (what, int(bad.sum()), bad.numel(), err.max().item())


def _gen(*key):
    return torch.Generator().manual_seed(7919 + sum(k * m for k, m in zip(key, (1, 131, 17161, 2248091))))


def _profiled(pkg, fn):
    pkg.ops.PROFILE = []
    try:
        out = fn()
        labels = [r[0] for r in pkg.ops.PROFILE]
    finally:
        pkg.ops.PROFILE = None
    return out, labels


@pytest.fixture
def guard(pkg, dev, monkeypatch):
    alloc = lp.GuardedAllocator().install(monkeypatch, pkg)
    yield alloc
    alloc.check()


@pytest.mark.parametrize('hw', SIZES, ids=['%dx%d' % s for s in SIZES])
@pytest.mark.parametrize('ch', CHANNELS, ids=['%dto%d' % c for c in CHANNELS])
def test_forward_and_weight_gradient(pkg, dev, ch, hw):
    """Forward with bias + residual + LeakyReLU, then its backward pass (the weight gradient runs wgrad4<thin_cout> for Cout <= 4); the forward a
    second time: bitwise equal."""
    (cin, cout), (h, w) = ch, hw
    g = _gen(cin, cout, h, w)
    x = torch.randn(2, cin, h, w, generator=g); wt = torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(cin * 9)
    b = torch.randn(cout, generator=g); rs = torch.randn(2, cout, h, w, generator=g)
    ref = [t.double().requires_grad_(True) for t in (x, wt, b, rs)]
    yr = F.leaky_relu(F.conv2d(ref[0], ref[1], ref[2], 1, 1) + ref[3], 0.2)
    dy = torch.randn(yr.shape, generator=g)
    yr.backward(dy.double())
    d = [t.to(dev).requires_grad_(True) for t in (x, wt, b, rs)]
    run = lambda: pkg.ops.conv2d(d[0], d[1], d[2], 1, 1, act=pkg._lib.ACT_LRELU, slope=0.2, res=d[3])
    yd, labels = _profiled(pkg, run)
    assert LABEL in labels, labels
    _, labels_b = _profiled(pkg, lambda: yd.backward(dy.to(dev)))
    if cout <= 4:                                      # wgrad4 takes <= 4 channels on the thin side; Cout 8 runs the wide weight gradient
        assert 'wgrad4_kernel<thin_cout>' in labels_b, labels_b
    what = '%d->%d %dx%d' % (cin, cout, h, w)
    _close(yd, yr, 1e-5, 2e-6 * math.sqrt(cin * 9), what + ' fwd')
    _close(d[1].grad, ref[1].grad, 2e-5, 2e-6 * math.sqrt(2 * h * w), what + ' wgrad')
    _close(d[2].grad, ref[2].grad, 2e-5, 1e-5, what + ' bias grad')
    with torch.no_grad():
        y2 = run()
    assert torch.equal(yd.detach(), y2), what + ': two forward launches differ'


@pytest.mark.parametrize('hw', SIZES, ids=['%dx%d' % s for s in SIZES])
@pytest.mark.parametrize('ch', CHANNELS, ids=['%dto%d' % c for c in CHANNELS])
def test_input_gradient(pkg, dev, ch, hw):
    """The input gradient of a `thin` -> `wide` layer: dy has `wide` channels, dx `thin` ones; twice: bitwise equal."""
    (wide, thin), (h, w) = ch, hw
    g = _gen(wide, thin, h, w, 1)
    x = torch.randn(2, thin, h, w, generator=g); wt = torch.randn(wide, thin, 3, 3, generator=g) / math.sqrt(thin * 9)
    dy = torch.randn(2, wide, h, w, generator=g)
    xr = x.double().requires_grad_(True)
    F.conv2d(xr, wt.double(), None, 1, 1).backward(dy.double())
    grads = []
    for _ in range(2):
        xd = x.to(dev).requires_grad_(True)
        yd = pkg.ops.conv2d(xd, wt.to(dev), None, 1, 1)
        _, labels = _profiled(pkg, lambda: yd.backward(dy.to(dev)))
        assert LABEL in labels, labels
        grads.append(xd.grad)
    what = 'dgrad of %d->%d %dx%d' % (thin, wide, h, w)
    _close(grads[0], xr.grad, 1e-5, 2e-6 * math.sqrt(wide * 9), what)
    assert torch.equal(grads[0], grads[1]), what + ': two launches differ'


@pytest.mark.parametrize('ch', [(64, 3), (128, 4), (64, 8)], ids=['64to3', '128to4', '64to8'])
def test_channel_slice_input_and_guarded_output(pkg, dev, guard, ch):
    """The input is a channel slice of a wider canary-filled buffer (pixel stride > C); the output comes from the guarded allocator:
    its pad lanes must be 0, the guard bands and the input's neighbouring lanes untouched, the values those of the compact run."""
    cin, cout = ch
    h, w = 9, 66
    g = _gen(cin, cout, 2)
    x = torch.randn(2, cin, h, w, generator=g); wt = torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(cin * 9)
    b = torch.randn(cout, generator=g)
    yr = F.conv2d(x.double(), wt.double(), b.double(), 1, 1)
    wd, bd = wt.to(dev), b.to(dev)
    with torch.no_grad():
        y0 = pkg.ops.conv2d(x.to(dev), wd, bd, 1, 1)
        for c0, ld in ((0, cin + 8), (4, cin + 8), (cin, 2 * cin)):
            xs = lp.poisoned_slice(x, ld, c0, dev)
            ys, labels = _profiled(pkg, lambda: pkg.ops.conv2d(xs, wd, bd, 1, 1))
            assert LABEL in labels, labels
            lp.check_slice(xs)
            guard.check()
            assert not torch.isnan(ys).any(), 'a neighbouring lane leaked into the result'
            _close(ys, yr, 1e-5, 2e-6 * math.sqrt(cin * 9), '%d->%d from lanes [%d, %d) of %d' % (cin, cout, c0, c0 + cin, ld))
            assert torch.equal(ys, y0), 'the channel slice changed the result'


def test_non_finite_inputs(pkg, dev):
    """One inf at an interior pixel and one nan at a corner: the non-finite outputs are where a float32 CPU convolution has them,
    the others meet the bound."""
    cin, cout, h, w = 64, 3, 9, 66
    g = _gen(cin, cout, 3)
    x = torch.randn(2, cin, h, w, generator=g); wt = torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(cin * 9)
    x[0, 5, 4, 31] = float('inf')
    x[1, 60, 0, 0] = float('nan')
    y32 = F.conv2d(x, wt, None, 1, 1)
    yr = F.conv2d(x.double(), wt.double(), None, 1, 1)
    with torch.no_grad():
        yd, labels = _profiled(pkg, lambda: pkg.ops.conv2d(x.to(dev), wt.to(dev), None, 1, 1))
    assert LABEL in labels, labels
    yd = yd.cpu()
    bad = ~torch.isfinite(yd)
    assert torch.equal(bad, ~torch.isfinite(y32)), 'non-finite outputs at other positions than the CPU convolution: %d vs %d' % (
        int(bad.sum()), int((~torch.isfinite(y32)).sum()))
    assert int(bad.sum()) == cout * (9 + 4)
    fin = ~bad
    _close(yd[fin], yr[fin], 1e-5, 2e-6 * math.sqrt(cin * 9), 'finite outputs next to inf / nan')
