"""The second switch of the bf16x1 discriminator: wgrad_s2='bf16x1' beside precision='bf16x1' moves the weight gradient of a 3x3
stride-2 pad-1 conv of the single-conv node onto wgrad_s2_k32_x1_kernel (ids 81 / 82) -- ops.conv2d(wgrad_s2=),
ops.conv2d_bf16x1_train(stride=2, wgrad_s2=), ops.train_precision(mode, wgrad_s2=) read by models_seg_gan.ConvolutionalBlock,
train_seg_gan.gan_step(d_wgrad_s2=).  Routing, wiring (bit-equality with the launcher) and mode handling only: the kernel's accuracy
is gated in tests/test_wgrad_s2_x1_gpu.py.  With the switch off everything is what tests/test_disc_x1_gpu.py pins."""
import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

S2_WGRAD = {128: 'wgrad_s2_k32_x1_kernel<128>', 64: 'wgrad_s2_k32_x1_kernel<64>'}
CLS64 = ['conv_s2_k32_x1_kernel<64,%d>' % t for t in (1, 2, 2, 4)]
_CACHE = {}


def _labels(pkg, fn, shapes=False):
    pkg.ops.PROFILE = []
    pkg.ops.PROFILE_SHAPES = shapes
    try:
        r = fn()
        torch.cuda.synchronize()
        return [rec[0] for rec in pkg.ops.PROFILE], r
    finally:
        pkg.ops.PROFILE = None
        pkg.ops.PROFILE_SHAPES = False


def _modes(pkg):
    return pkg.ops.train_precision_mode(), pkg.ops.train_wgrad_s2_mode()


def test_single_conv_wiring(pkg, dev):
    ops = pkg.ops
    assert ops._WGRAD_X1_S2_LABELS == {81: S2_WGRAD[128], 82: S2_WGRAD[64]}

    def run(**kw):
        g = torch.Generator().manual_seed(8)
        x = (torch.randn(2, 64, 19, 38, generator=g) * 1.5 + 0.3).to(dev).requires_grad_(True)
        w = (torch.randn(128, 64, 3, 3, generator=g) / 24).to(dev).requires_grad_(True)
        b = torch.randn(128, generator=g).to(dev).requires_grad_(True)
        dout = torch.randn(2, 128, 10, 19, generator=g).to(dev)
        fwd, y = _labels(pkg, lambda: ops.conv2d(x, w, b, stride=2, padding=1, precision='bf16x1', **kw))
        bwd, _ = _labels(pkg, lambda: y.backward(dout))
        return fwd, bwd, x, w, b, dout, y.detach()

    fwd, bwd, x, w, b, dout, y = run(wgrad_s2='bf16x1')
    fwd0, bwd0, x0, w0, b0, _, y0 = run()
    assert fwd == fwd0 == ['conv_s2_k32_x1_kernel<128,9>']
    assert bwd == CLS64 + [S2_WGRAD[128]], bwd
    assert bwd0[:4] == CLS64 and len(bwd0) == 5 and '_x1_' not in bwd0[4], bwd0
    with torch.no_grad():
        xn, dyn = ops.to_nhwc(x.detach()), ops.to_nhwc(dout)
        dw = ops._conv_wgrad_s2_bf16x1_impl(xn, dyn, w.shape)
        assert dw is not None and torch.equal(w.grad, dw)
        assert torch.equal(w0.grad, ops._conv_wgrad_impl(xn, None, dyn, w.shape, 2, 1))
    assert torch.equal(y, y0) and torch.equal(x.grad, x0.grad) and torch.equal(b.grad, b0.grad)
    assert not torch.equal(w.grad, w0.grad)
    # the differentiable entry point with stride=2 is the same node
    x2 = x.detach().clone().requires_grad_(True)
    w2 = w.detach().clone().requires_grad_(True)
    ops.conv2d_bf16x1_train(x2, w2, b.detach(), stride=2, wgrad_s2='bf16x1').backward(dout)
    assert torch.equal(w2.grad, w.grad) and torch.equal(x2.grad, x.grad)
    w3 = w.detach().clone().requires_grad_(True)
    ops.conv2d_bf16x1_train(x.detach(), w3, b.detach(), stride=2).backward(dout)
    assert torch.equal(w3.grad, w0.grad)


def test_refused_shape_runs_todays_kernel(pkg, dev):
    ops = pkg.ops
    g = torch.Generator().manual_seed(9)
    x = torch.randn(1, 48, 12, 40, generator=g).to(dev)
    dout = torch.randn(1, 64, 6, 20, generator=g).to(dev)
    got = []
    for kw in (dict(wgrad_s2='bf16x1'), dict()):
        w = (torch.randn(64, 48, 3, 3, generator=torch.Generator().manual_seed(10)) / 20).to(dev).requires_grad_(True)
        y = ops.conv2d(x, w, None, stride=2, padding=1, precision='bf16x1', **kw)
        labels, _ = _labels(pkg, lambda: y.backward(dout))
        got.append((labels, w.grad.clone()))
    assert got[0][0] == got[1][0] and len(got[0][0]) == 1 and '_x1_' not in got[0][0][0], got[0][0]
    assert torch.equal(got[0][1], got[1][1])
    with torch.no_grad():
        assert ops._conv_wgrad_s2_bf16x1_impl(ops.to_nhwc(x), ops.to_nhwc(dout), (64, 48, 3, 3)) is None


def test_value_errors_and_restored_modes(pkg, dev):
    ops = pkg.ops
    x = torch.randn(1, 64, 8, 40, device=dev)
    w = torch.randn(64, 64, 3, 3, device=dev)
    for kw in (dict(precision='fp32', wgrad_s2='bf16x1'), dict(wgrad_s2='bf16x1'), dict(precision='bf16x1', wgrad_s2='bf16'),
               dict(precision='bf16x1', wgrad_s2=None)):
        with pytest.raises(ValueError):
            ops.conv2d(x, w, None, stride=2, padding=1, **kw)
    with pytest.raises(ValueError):
        ops.conv2d_bf16x1_train(x, w, None, stride=2, wgrad_s2='bf16')
    for args, kw in ((('fp32',), dict(wgrad_s2='bf16x1')), (('bf16x1',), dict(wgrad_s2='x1')), (('bf16',), dict())):
        with pytest.raises(ValueError):
            ops.train_precision(*args, **kw)
    for kw in (dict(d_wgrad_s2='bf16x1'), dict(d_precision='fp32', d_wgrad_s2='bf16x1'), dict(d_precision='bf16x1', d_wgrad_s2='fp16'),
               dict(precision='bf16x1', d_wgrad_s2='bf16x1')):
        with pytest.raises(ValueError):
            pkg.train_seg_gan.gan_step(None, None, None, None, None, None, None, None, None, 3, **kw)
    assert _modes(pkg) == ('fp32', 'fp32')
    with ops.train_precision('bf16x1', wgrad_s2='bf16x1'):
        assert _modes(pkg) == ('bf16x1', 'bf16x1')
        with ops.train_precision('bf16x1'):
            assert _modes(pkg) == ('bf16x1', 'fp32')
        with ops.train_precision('fp32'):
            assert _modes(pkg) == ('fp32', 'fp32')
        assert _modes(pkg) == ('bf16x1', 'bf16x1')
    assert _modes(pkg) == ('fp32', 'fp32')
    with pytest.raises(TypeError):
        ops.infer_precision('bf16x1', wgrad_s2='bf16x1')       # the inference context does not grow the argument


# ----------------------------------------------------------------------------- the discriminator under train_precision
def _disc_run(pkg, dev, wgrad_s2):
    """Forward + backward of Discriminator(3, 3, 64, 4, 1024) on 1 x 3 x 68 x 68 (levels 68 -> 34 -> 17) under 'bf16x1':
    (forward labels, backward labels, tensors); labels carry the launch geometry."""
    if wgrad_s2 in _CACHE:
        return _CACHE[wgrad_s2]
    torch.manual_seed(5)
    D = pkg.models_seg_gan.Discriminator(3, 3, 64, 4, 1024).to(dev).train()
    x = torch.randn(1, 3, 68, 68, generator=torch.Generator().manual_seed(6)).to(dev).requires_grad_(True)
    with pkg.ops.train_precision('bf16x1', **({} if wgrad_s2 is None else dict(wgrad_s2=wgrad_s2))):
        fwd, out = _labels(pkg, lambda: D(x), shapes=True)
    bwd, _ = _labels(pkg, lambda: out.sum().backward(), shapes=True)
    got = [out.detach().cpu(), x.grad.cpu()] + [p.grad.cpu() for p in D.parameters()]
    _CACHE[wgrad_s2] = (fwd, bwd, got, [tuple(p.shape) for p in D.parameters()])
    return _CACHE[wgrad_s2]


def test_discriminator_routing_labels(pkg, dev):
    fwd, bwd, t, shapes = _disc_run(pkg, dev, 'bf16x1')
    fwd0, bwd0, t0, _ = _disc_run(pkg, dev, None)
    fwd1, bwd1, t1, _ = _disc_run(pkg, dev, 'fp32')
    assert fwd0 == fwd1 and bwd0 == bwd1 and all(torch.equal(a, b) for a, b in zip(t0, t1))       # 'fp32' given = omitted
    assert fwd == fwd0 and len(bwd) == len(bwd0)
    changed = [(a, b) for a, b in zip(bwd0, bwd) if a != b]
    name = lambda l: l.split(' n1 ')[0]
    geo = lambda l: l.split(' n1 ')[1]
    # exactly the two stride-2 weight gradients change label, the deeper layer (128 -> 128 at 34^2 -> 17^2) first; geometry as before
    assert [name(b) for _, b in changed] == [S2_WGRAD[128], S2_WGRAD[64]], changed
    assert all(geo(a) == geo(b) and ' k3 s2' in a and '_x1_' not in a for a, b in changed), changed
    assert [geo(b) for _, b in changed] == ['17x17 cin128 cout128 k3 s2', '34x34 cin64 cout64 k3 s2'], changed
    stem = lambda ls: [l for l in ls if ' cin3 ' in l or ' cout3 ' in l]
    assert stem(bwd) == stem(bwd0) and stem(bwd) and not any('_x1_' in l for l in stem(bwd))
    # the forward, the input gradient and every other parameter gradient keep their bits; the two stride-2 weights move
    moved = [i for i, (a, b) in enumerate(zip(t0, t)) if not torch.equal(a, b)]
    s2_weights = [2 + i for i, s in enumerate(shapes) if s in ((64, 64, 3, 3), (128, 128, 3, 3))]
    assert len(s2_weights) == 2 and moved == s2_weights, (moved, s2_weights)


# ----------------------------------------------------------------------------- gan_step
def _two_steps(pkg, dev, key, **kw):
    if key in _CACHE:
        return _CACHE[key]
    from oracle import seg_gan_cpu as O
    inp, tgt = O.synthetic_batch(2, 64, 64)
    torch.manual_seed(41)
    G = pkg.models_seg_gan.Generator(dict(arch='UNet_R_SS_v2', num_classes=3, input_channels=3, deep_supervision=False))
    D = pkg.models_seg_gan.Discriminator(3, 3, 64, 8, 1024)
    G.to(dev).train(); D.to(dev).train()
    og = torch.optim.Adam(G.parameters(), lr=2e-5); od = torch.optim.Adam(D.parameters(), lr=2e-5)
    scal = []

    def steps():
        for _ in range(2):
            scal.append(pkg.train_seg_gan.gan_step(inp.to(dev), tgt.to(dev), G, D, pkg.losses.BCEDiceLoss(), nn.BCEWithLogitsLoss(), nn.MSELoss(),
                                                   og, od, 3, **kw))
    labels, _ = _labels(pkg, steps)
    out = ([p.detach().cpu().clone() for p in G.parameters()], [p.detach().cpu().clone() for p in D.parameters()],
           [[float(v) for v in s] for s in scal], labels)
    _CACHE[key] = out
    return out


@pytest.mark.parametrize('d_precision', ['fp32', 'bf16x1'])
def test_gan_step_d_wgrad_s2_fp32_is_the_default(pkg, dev, d_precision):
    g0, d0, s0, l0 = _two_steps(pkg, dev, ('omitted', d_precision), d_precision=d_precision)
    g1, d1, s1, l1 = _two_steps(pkg, dev, ('given', d_precision), d_precision=d_precision, d_wgrad_s2='fp32')
    assert s0 == s1 and l0 == l1
    assert all(torch.equal(a, b) for a, b in zip(g0 + d0, g1 + d1))
    assert not any(l.startswith('wgrad_s2_k32_x1') for l in l0)


def test_gan_step_d_wgrad_s2_bf16x1(pkg, dev):
    _, dd, s, labels = _two_steps(pkg, dev, ('s2', 'bf16x1'), d_precision='bf16x1', d_wgrad_s2='bf16x1')
    _, dd0, _, labels0 = _two_steps(pkg, dev, ('omitted', 'bf16x1'), d_precision='bf16x1')
    assert len(s) == 2 and all(len(v) == 6 and all(np.isfinite(x) for x in v) for v in s), s
    # at 64^2 only the 64^2 -> 32^2 stride-2 layer is legal: the other stride-2 weight gradients fall back per launch
    assert S2_WGRAD[64] in labels and S2_WGRAD[128] not in labels, set(labels)
    # every other launch of the two steps, the generator's among them, is what it was
    assert len(labels) == len(labels0)
    diff = [(a, b) for a, b in zip(labels0, labels) if a != b]
    assert diff and all(b == S2_WGRAD[64] and a.startswith('wgrad_') and '_x1' not in a for a, b in diff), diff
    assert any(not torch.equal(a, b) for a, b in zip(dd0, dd)), 'the step with the switch on equals the step without it'
    assert (pkg.ops.train_precision_mode(), pkg.ops.train_wgrad_s2_mode()) == ('fp32', 'fp32')
