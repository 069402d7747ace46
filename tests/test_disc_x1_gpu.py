"""ops.train_precision('bf16x1') on the discriminator: models_seg_gan.ConvolutionalBlock hands the mode to ops.conv2d(precision=),
whose single-conv node asks the one-term kernels first -- ids 70 / 71 / 72 for the stride-1 layers, conv_s2_k32_x1_kernel for the
stride-2 forward and input gradient -- and runs today's kernel where they refuse; train_seg_gan.gan_step(d_precision=...).
Routing, wiring (bit-equality with direct launcher calls) and mode handling only: the kernels' accuracy is gated in
tests/test_conv_s2_bf16x1_gpu.py, tests/test_conv_bf16x1_gpu.py and tests/test_wgrad_x1_gpu.py."""
import contextlib

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

X1_CONV = ('conv_halo_k32_x1_kernel<128>', 'conv_halo_k32_x1_kernel<64>')
X1_WGRAD = 'wgrad_k32_x1_kernel'
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


def _disc_run(pkg, dev, precision):
    """Forward + backward of Discriminator(3, 3, 64, 4, 1024) on 1 x 3 x 68 x 68 (levels 68 -> 34 -> 17: every layer but the stem is
    legal): (forward labels, backward labels, tensors).  Labels carry the launch geometry; the two linear layers are filtered out."""
    if precision in _CACHE:
        return _CACHE[precision]
    torch.manual_seed(5)
    D = pkg.models_seg_gan.Discriminator(3, 3, 64, 4, 1024).to(dev).train()
    x = torch.randn(1, 3, 68, 68, generator=torch.Generator().manual_seed(6)).to(dev).requires_grad_(True)
    ctx = pkg.ops.train_precision(precision) if precision else contextlib.nullcontext()
    with ctx:
        fwd, out = _labels(pkg, lambda: D(x), shapes=True)
    bwd, _ = _labels(pkg, lambda: out.sum().backward(), shapes=True)
    conv = lambda ls: [l for l in ls if ' taps9 ' in l or ' s1/2' in l or ' k3 ' in l]
    got = [out.detach().cpu(), x.grad.cpu()] + [p.grad.cpu() for p in D.parameters()]
    _CACHE[precision] = (conv(fwd), conv(bwd), got)
    return _CACHE[precision]


def test_discriminator_routing_labels(pkg, dev):
    ops = pkg.ops
    fwd, bwd, _ = _disc_run(pkg, dev, 'bf16x1')
    fwd0, bwd0, _ = _disc_run(pkg, dev, None)
    name = lambda l: l.split(' n1 ')[0]
    # forward: the 3 -> 64 stem on its old kernel, then the new stride-2 id, id 70, the new stride-2 id
    assert len(fwd) == 4 and name(fwd[0]) == name(fwd0[0]) and '_x1_' not in fwd[0], fwd
    assert [name(l) for l in fwd[1:]] == ['conv_s2_k32_x1_kernel<64,9>', X1_CONV[0], 'conv_s2_k32_x1_kernel<128,9>'], fwd
    # backward: stride-1 input and weight gradients on 70 / 71 and 72, stride-2 input gradients on the class ids, stride-2 weight
    # gradients (and everything of the stem) on today's ids
    cls128 = ['conv_s2_k32_x1_kernel<128,%d>' % t for t in (1, 2, 2, 4)]
    cls64 = ['conv_s2_k32_x1_kernel<64,%d>' % t for t in (1, 2, 2, 4)]
    assert [name(l) for l in bwd if 'conv_s2' in l] == cls128 + cls64, bwd
    assert [name(l) for l in bwd if name(l) in X1_CONV] == [X1_CONV[1]], bwd                   # dx of 64 -> 128 has 64 rows
    assert [name(l) for l in bwd].count(X1_WGRAD) == 1, bwd
    old = lambda ls: sorted(l for l in ls if '_x1_' not in l and ' s2' in l and ' k3 ' in l)
    assert len(old(bwd)) == 2 and old(bwd) == old(bwd0), (bwd, bwd0)                            # the two stride-2 weight gradients
    stem = lambda ls: sorted(l for l in ls if ' cin3 ' in l or ' cout3 ' in l)
    assert stem(bwd) == stem(bwd0) and stem(bwd), (bwd, bwd0)
    assert not any('_x1_' in l for l in fwd0 + bwd0)
    assert set(ops._X1_LABELS) == {70, 71} and set(ops._X1_S2_LABELS) == {73, 74} and set(ops._X1_CLS_LABELS) == set(range(75, 81))


def test_mode_fp32_is_bit_identical_to_no_context(pkg, dev):
    f0, b0, t0 = _disc_run(pkg, dev, None)
    f1, b1, t1 = _disc_run(pkg, dev, 'fp32')
    assert f0 == f1 and b0 == b1
    assert all(torch.equal(a, b) for a, b in zip(t0, t1))
    _, _, tx = _disc_run(pkg, dev, 'bf16x1')
    assert not all(torch.equal(a, b) for a, b in zip(t0, tx))


def test_stride2_node_wiring(pkg, dev):
    """One stride-2 _Conv2d under 'bf16x1': y and dx are the new launchers' bits, dw is _conv_wgrad_impl's on the unrounded x, dy,
    db is _channel_sum's."""
    ops = pkg.ops
    g = torch.Generator().manual_seed(8)
    x = (torch.randn(2, 64, 19, 38, generator=g) * 1.5 + 0.3).to(dev).requires_grad_(True)
    w = (torch.randn(128, 64, 3, 3, generator=g) / 24).to(dev).requires_grad_(True)
    b = torch.randn(128, generator=g).to(dev).requires_grad_(True)
    dout = torch.randn(2, 128, 10, 19, generator=g).to(dev)
    labels, y = _labels(pkg, lambda: ops.conv2d(x, w, b, stride=2, padding=1, precision='bf16x1'))
    assert labels == ['conv_s2_k32_x1_kernel<128,9>']
    labels, _ = _labels(pkg, lambda: y.backward(dout))
    assert labels[:4] == ['conv_s2_k32_x1_kernel<64,%d>' % t for t in (1, 2, 2, 4)] and len(labels) == 5 and '_x1_' not in labels[4], labels
    with torch.no_grad():
        xn, dyn = ops.to_nhwc(x.detach()), ops.to_nhwc(dout)
        assert torch.equal(y.detach(), ops._conv_s2_bf16x1_impl(xn, w.detach(), b.detach(), 0, 0.0))
        assert torch.equal(x.grad, ops._conv_dgrad_s2_bf16x1_impl(dyn, w.detach(), 19, 38, 0, 64))
        assert torch.equal(w.grad, ops._conv_wgrad_impl(xn, None, dyn, w.shape, 2, 1))
        assert torch.equal(b.grad, ops._channel_sum(dyn, 128))
    # the differentiable entry point with stride=2 is the same node
    x2 = x.detach().clone().requires_grad_(True)
    y2 = ops.conv2d_bf16x1_train(x2, w.detach(), b.detach(), stride=2)
    y2.backward(dout)
    assert torch.equal(y2.detach(), y.detach()) and torch.equal(x2.grad, x.grad)


def test_basic_block_launches_what_it_launched(pkg, dev):
    """The block nodes never ask the stride-2 route and keep their own: a two-input BasicBlock (64 + 64 -> 128 on 6 x 33, 1x1
    shortcut) under 'bf16x1' launches the list tests/test_train_x1_gpu.py::test_routing_labels pins -- five launches on ids 70 / 71,
    two on id 72, four (the shortcut's) on old ids -- and none of the stride-2 ids."""
    torch.manual_seed(3)
    blk = pkg.archs.BasicBlock(128, 128).to(dev).train()
    if not len(blk.shortcut):
        blk.shortcut = nn.Sequential(nn.Conv2d(128, 128, kernel_size=1, bias=False)).to(dev)
    g = torch.Generator().manual_seed(4)
    x1 = torch.randn(2, 64, 6, 33, generator=g).to(dev).requires_grad_(True)
    x2 = torch.randn(2, 64, 6, 33, generator=g).to(dev).requires_grad_(True)

    def run():
        with pkg.ops.train_precision('bf16x1'):
            blk(x1, x2).sum().backward()
    labels, _ = _labels(pkg, run)
    assert sum(l in X1_CONV for l in labels) == 5 and labels.count(X1_WGRAD) == 2, labels
    others = [l for l in labels if l not in X1_CONV and l != X1_WGRAD]
    assert len(others) == 4 and '?' not in others and not any('conv_s2' in l for l in labels), labels


# ----------------------------------------------------------------------------- gan_step
def _two_steps(pkg, dev, key, *extra, **kw):
    if key in _CACHE:
        return _CACHE[key]
    from oracle import seg_gan_cpu as O
    inp, tgt = O.synthetic_batch(2, 64, 64)
    torch.manual_seed(41)
    G = pkg.models_seg_gan.Generator(dict(arch='UNet_R_SS_v2', num_classes=3, input_channels=3, deep_supervision=False))
    D = pkg.models_seg_gan.Discriminator(3, 3, 64, 8, 1024)
    G.to(dev).train(); D.to(dev).train()
    d0 = [p.detach().cpu().clone() for p in D.parameters()]
    og = torch.optim.Adam(G.parameters(), lr=2e-5); od = torch.optim.Adam(D.parameters(), lr=2e-5)
    scal = []

    def steps():
        for _ in range(2):
            scal.append(pkg.train_seg_gan.gan_step(inp.to(dev), tgt.to(dev), G, D, pkg.losses.BCEDiceLoss(), nn.BCEWithLogitsLoss(), nn.MSELoss(),
                                                   og, od, 3, *extra, **kw))
    labels, _ = _labels(pkg, steps)
    out = (d0, [p.detach().cpu().clone() for p in G.parameters()], [p.detach().cpu().clone() for p in D.parameters()],
           [[float(v) for v in s] for s in scal], labels)
    _CACHE[key] = out
    return out


@pytest.mark.parametrize('precision', ['fp32', 'bf16x1'])
def test_gan_step_d_precision_fp32_is_the_default(pkg, dev, precision):
    _, g0, dd0, s0, l0 = _two_steps(pkg, dev, ('default', precision), None, None, precision)          # sync_g, sync_d, precision: positional
    _, g1, dd1, s1, l1 = _two_steps(pkg, dev, ('d_fp32', precision), precision=precision, d_precision='fp32')
    assert s0 == s1 and l0 == l1
    assert all(torch.equal(a, b) for a, b in zip(g0 + dd0, g1 + dd1))
    assert not any('conv_s2' in l for l in l0)


def test_gan_step_d_precision_bf16x1(pkg, dev):
    d0, _, dd, s, labels = _two_steps(pkg, dev, ('d_x1', 'fp32'), d_precision='bf16x1')
    _, _, dd_fp32, _, _ = _two_steps(pkg, dev, ('default', 'fp32'), None, None, 'fp32')
    assert len(s) == 2 and all(len(v) == 6 and all(np.isfinite(x) for x in v) for v in s), s
    # the generator is fp32 here: every one-term launch is the discriminator's
    assert sum(l in X1_CONV for l in labels) > 0 and labels.count(X1_WGRAD) > 0
    # at 64^2 only the 64^2 -> 32^2 stride-2 layer is legal: the others fall back per launch
    assert 'conv_s2_k32_x1_kernel<64,9>' in labels and 'conv_s2_k32_x1_kernel<64,4>' in labels
    assert not any(l.startswith('conv_s2_k32_x1_kernel<128') for l in labels), set(labels)
    assert all(not torch.equal(a, b) for a, b in zip(d0, dd) if a.dim() == 4), 'a discriminator conv weight did not move'
    assert any(not torch.equal(a, b) for a, b in zip(dd_fp32, dd)), 'the bf16x1 discriminator step equals the fp32 step'
    assert pkg.ops.train_precision_mode() == 'fp32'


def test_gan_step_refuses_an_unknown_d_precision(pkg, dev):
    with pytest.raises(ValueError):
        pkg.train_seg_gan.gan_step(None, None, None, None, None, None, None, None, None, 3, d_precision='bf16')
    assert pkg.ops.train_precision_mode() == 'fp32'
