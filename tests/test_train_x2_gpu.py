"""ops.train_precision('bf16x2') / ops.infer_precision('bf16x2') at module level: archs.BasicBlock (train node, frozen node, eval
path), train_seg_gan.gan_step(precision='bf16x2') and segment_image(precision='bf16x2') on the two-term kernels (ids 90 / 91 / 92).

The accuracy gate is RELATIVE, so no absolute tolerance is invented: per output and gradient tensor of a BasicBlock (the cases of
tests/train_x1_ref.py: 2 x 64 -> 64 on 8 x 24 with the identity shortcut, 2 x (64 + 64) -> 128 on 6 x 33 with the 1x1 shortcut), the
RMS difference between the 'bf16x2' run and the fp32-class run on the same data is at most 1/16 of the difference of the 'bf16x1'
run.  Theory puts the ratio near 2^-8 (tests/test_bf16x2_ref.py measures 0.0019 on the quantised fp64 blocks); the factor 16 is
slack for an isolated ReLU flip."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import train_x1_ref as tr
from test_train_x1_gpu import _build, _labels, _run, _same

pytestmark = pytest.mark.gpu

X2_CONV = ('conv_halo_k32_x2_kernel<128>', 'conv_halo_k32_x2_kernel<64>')
X2_WGRAD = 'wgrad_k32_x2_kernel'
X1_ALL = ('conv_halo_k32_x1_kernel<128>', 'conv_halo_k32_x1_kernel<64>', 'wgrad_k32_x1_kernel')


def _three(pkg, dev, case, mode):
    runs = {}
    for precision in ('fp32', 'bf16x1', 'bf16x2'):
        blk, x1, x2, dout = _build(pkg, dev, case, mode)
        runs[precision] = _labels(pkg, lambda: _run(pkg, blk, dev, x1, x2, dout, precision))
    return runs


@pytest.mark.parametrize('case', sorted(tr.CASES))
def test_train_block_routes_and_is_16x_closer_than_one_term(pkg, dev, case):
    runs = _three(pkg, dev, case, 'train')
    labels, got = runs['bf16x2']
    nconv = 5 if case == 'cat128' else 4                   # two forwards, dy1, dx1 (and dx2 of the concat input)
    assert sum(l in X2_CONV for l in labels) == nconv and labels.count(X2_WGRAD) == 2, labels
    assert not any(l in X1_ALL for l in labels)
    others = [l for l in labels if l not in X2_CONV and l != X2_WGRAD]
    assert len(others) == (4 if case == 'cat128' else 0) and '?' not in others, labels       # the 1x1 shortcut: its fp32-class kernels
    base, one = runs['fp32'][1], runs['bf16x1'][1]
    assert set(others) <= set(runs['fp32'][0])
    bad = []
    for k in sorted(got):
        r2 = float((got[k].double() - base[k].double()).pow(2).mean().sqrt())
        r1 = float((one[k].double() - base[k].double()).pow(2).mean().sqrt())
        print('RATIO %-7s %-3s rms(bf16x2 - fp32) %.3e  rms(bf16x1 - fp32) %.3e  ratio %s' % (case, k, r2, r1, '%.5f' % (r2 / r1) if r1 else 'n/a'))
        if not r2 <= r1 / 16:
            bad.append((k, r2, r1))
    assert not bad, bad


@pytest.mark.parametrize('case', sorted(tr.CASES))
def test_frozen_block_routes(pkg, dev, case):
    blk, x1, x2, dout = _build(pkg, dev, case, 'frozen')
    labels, got = _labels(pkg, lambda: _run(pkg, blk, dev, x1, x2, dout, 'bf16x2'))
    nconv = 5 if case == 'cat128' else 4
    assert sum(l in X2_CONV for l in labels) == nconv and labels.count(X2_WGRAD) == 2, labels
    assert not any(l in X1_ALL for l in labels)
    blk, x1, x2, dout = _build(pkg, dev, case, 'frozen')
    base = _run(pkg, blk, dev, x1, x2, dout, 'fp32')
    assert all(torch.isfinite(v).all() for v in got.values()) and not _same(got, base)


def test_eval_block_honours_infer_precision(pkg, dev):
    blk, x1, x2, _ = _build(pkg, dev, 'cat128', 'train')
    blk.eval()
    a, b = x1.to(dev), x2.to(dev)
    with torch.no_grad():
        base = blk(a, b)
        with pkg.ops.infer_precision('bf16x2'):
            labels, got = _labels(pkg, lambda: blk(a, b))
        with pkg.ops.infer_precision('bf16x1'):
            one = blk(a, b)
    assert sum(l in X2_CONV for l in labels) == 2 and not any(l in X1_ALL for l in labels), labels
    r2 = float((got - base).double().pow(2).mean().sqrt()); r1 = float((one - base).double().pow(2).mean().sqrt())
    assert 0 < r2 <= r1 / 16, (r2, r1)
    assert pkg.ops.infer_precision_mode() == 'fp32'


def test_conv2d_precision_bf16x2_falls_back_per_launch(pkg, dev):
    ops = pkg.ops
    g = torch.Generator().manual_seed(5)
    w = (torch.randn(64, 64, 3, 3, generator=g) / 24).to(dev).requires_grad_(True)
    # stride 2 and a 16-pixel-wide image stay on the fp32-class kernels, bit for bit
    for x, stride in ((torch.randn(1, 64, 20, 20, generator=g), 2), (torch.randn(1, 64, 8, 16, generator=g), 1)):
        outs = []
        for precision in ('fp32', 'bf16x2'):
            xd = x.to(dev).requires_grad_(True)
            w.grad = None
            labels, y = _labels(pkg, lambda: ops.conv2d(xd, w, None, stride, 1, precision=precision))
            l2, _ = _labels(pkg, lambda: y.sum().backward())
            assert not any(l in X2_CONV or l == X2_WGRAD for l in labels + l2)
            outs.append((y.detach().cpu(), xd.grad.cpu(), w.grad.cpu().clone()))
        assert all(torch.equal(p, q) for p, q in zip(*outs))
    xd = torch.randn(1, 64, 8, 20, generator=g).to(dev).requires_grad_(True)
    labels, y = _labels(pkg, lambda: ops.conv2d(xd, w, None, 1, 1, precision='bf16x2'))
    l2, _ = _labels(pkg, lambda: y.sum().backward())
    assert labels == [X2_CONV[1]] and sorted(l2) == sorted([X2_CONV[1], X2_WGRAD]), (labels, l2)
    with pytest.raises(ValueError):
        ops.conv2d(xd, w, None, 1, 1, precision='bf16x2', wgrad_s2='bf16x1')
    for bad in ('bf16', 'medium', 'x1', 'fp16'):
        with pytest.raises(ValueError):
            ops.conv2d(xd, w, None, 1, 1, precision=bad)
        with pytest.raises(ValueError):
            ops.train_precision(bad)
        with pytest.raises(ValueError):
            ops.infer_precision(bad)


def _one_step(pkg, dev, *extra, **kw):
    from oracle import seg_gan_cpu as O
    inp, tgt = O.synthetic_batch(2, 64, 64)
    torch.manual_seed(41)
    G = pkg.models_seg_gan.Generator(dict(arch='UNet_R_SS_v2', num_classes=3, input_channels=3, deep_supervision=False))
    D = pkg.models_seg_gan.Discriminator(3, 3, 64, 8, 1024)
    G.to(dev).train(); D.to(dev).train()
    og = torch.optim.Adam(G.parameters(), lr=2e-5); od = torch.optim.Adam(D.parameters(), lr=2e-5)
    s = pkg.train_seg_gan.gan_step(inp.to(dev), tgt.to(dev), G, D, pkg.losses.BCEDiceLoss(), nn.BCEWithLogitsLoss(), nn.MSELoss(),
                                   og, od, 3, *extra, **kw)
    torch.cuda.synchronize()
    return [float(v) for v in s], [p.detach().cpu().clone() for p in list(G.parameters()) + list(D.parameters())]


def test_gan_step_three_precisions(pkg, dev):
    s_base, p_base = _one_step(pkg, dev)
    s_fp32, p_fp32 = _one_step(pkg, dev, precision='fp32')
    assert s_base == s_fp32 and all(torch.equal(a, b) for a, b in zip(p_base, p_fp32)), "precision='fp32' differs from the positional default"
    s_x1, _ = _one_step(pkg, dev, precision='bf16x1')
    labels, (s_x2, p_x2) = _labels(pkg, lambda: _one_step(pkg, dev, precision='bf16x2'))
    assert sum(l in X2_CONV for l in labels) > 0 and labels.count(X2_WGRAD) > 0 and not any(l in X1_ALL for l in labels)
    for s in (s_base, s_x1, s_x2):
        assert len(s) == 6 and all(np.isfinite(v) for v in s), s
    # loss, content loss and the two adversarial losses of the first step (iou / dice are thresholded counts)
    d2 = [abs(s_x2[i] - s_base[i]) for i in (0, 3, 4, 5)]
    d1 = [abs(s_x1[i] - s_base[i]) for i in (0, 3, 4, 5)]
    print('gan_step scalars |bf16x2 - fp32| %s  |bf16x1 - fp32| %s' % (d2, d1))
    assert all(a <= b for a, b in zip(d2, d1)) and sum(d2) < sum(d1), (d2, d1)
    assert any(not torch.equal(a, b) for a, b in zip(p_base, p_x2)), 'the bf16x2 step equals the fp32 step'
    with pytest.raises(ValueError, match='d_precision'):
        _one_step(pkg, dev, precision='bf16x2', d_precision='bf16x2')
    assert pkg.ops.train_precision_mode() == 'fp32'


def test_segment_image_bf16x2(pkg, dev):
    from test_infer_bf16x1_gpu import _perturb_stats
    A = pkg.aerial_image_segmentation_api
    torch.manual_seed(41)
    model = pkg.archs.UNet_R_SS_v2(3, 3, False).to(dev).eval()
    _perturb_stats(model, 6)
    img = np.random.default_rng(21).integers(0, 256, (96, 96, 3), dtype=np.uint8)
    cfg = dict(patch_size=64, input_w=64, input_h=64, patch_overlap=0.5, num_classes=3)
    base = A.segment_image(model, img, cfg, batch_size=4)
    labels, got = _labels(pkg, lambda: A.segment_image(model, img, cfg, batch_size=4, precision='bf16x2'))
    assert any(l in X2_CONV for l in labels) and not any(l in X1_ALL for l in labels)
    assert len(got) == 3
    for m in got:
        assert m.dtype == np.uint8 and m.shape == (96, 96) and set(np.unique(m)) <= {0, 255}
    print('segment_image: %.4f %% of mask bytes differ between fp32 and bf16x2' % (100 * np.mean([np.mean(a != b) for a, b in zip(base, got)])))
    xc = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(9))
    p2 = A.infer_patches(model, xc, batch_size=2, precision='bf16x2')
    assert torch.equal(p2, A.infer_patches(model, xc, batch_size=2, graph=True, precision='bf16x2'))
    full = A.segmentation_inference_full
    assert 'precision' in full.__code__.co_varnames
    for bad in ('bf16', 'medium', 'x1', 'fp16'):
        with pytest.raises(ValueError):
            A.segment_image(model, img, cfg, precision=bad)
    assert pkg.ops.infer_precision_mode() == 'fp32'
