"""`ops.infer_precision('bf16x1')` through the eval-mode BasicBlock, the generator and the inference API.  The REFERENCE is the
project's existing fp32-class kernels fed bf16-rounded operands, never the new kernel: inside a test `ops.conv2d_bf16x1` is
replaced by a function that rounds x, x2 and the weight on the device and calls `ops.conv2d`.  EMU = that, X1 = the new path,
FP32 = the default path.  Caps: |X1 - FP32| <= 1.5 x |EMU - FP32| in max and 1.25 x in rms (the CPU stand-in sits at 1.00,
tests/test_bf16x1_ref.py; truncation instead of rounding doubles the rms, a lost product term raises the max severalfold)."""
import numpy as np
import pytest
import torch

import bf16x1_ref as R

pytestmark = pytest.mark.gpu


def _emu(ops):
    rnd = lambda t: None if t is None else t.bfloat16().float()

    def conv2d_bf16x1(x, weight, bias=None, act=0, slope=0.0, x2=None, res=None):
        return ops.conv2d(rnd(x), rnd(weight), bias, 1, 1, act=act, slope=slope, x2=rnd(x2), res=res)
    return conv2d_bf16x1


def _perturb_stats(model, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                c = m.num_features
                m.running_mean.copy_(torch.randn(c, generator=g) * 0.3)
                m.running_var.copy_(0.5 + torch.rand(c, generator=g))
                if m.affine:                                 # SPADE's parameter-free norms have no weight / bias
                    m.weight.copy_(0.5 + torch.rand(c, generator=g))
                    m.bias.copy_(torch.randn(c, generator=g) * 0.2)


def _three_paths(pkg, monkeypatch, run):
    """(FP32, X1, EMU, labels of the FP32 run, labels of the X1 run) of `run()`."""
    ops = pkg.ops
    with torch.no_grad():
        ops.PROFILE = []
        try:
            fp32 = run().clone(); l32 = [p[0] for p in ops.PROFILE]
            ops.PROFILE = []
            with ops.infer_precision('bf16x1'):
                x1 = run().clone()
            lx1 = [p[0] for p in ops.PROFILE]
        finally:
            ops.PROFILE = None
        with monkeypatch.context() as mp:
            mp.setattr(ops, 'conv2d_bf16x1', _emu(ops))
            with ops.infer_precision('bf16x1'):
                emu = run().clone()
    assert ops.infer_precision_mode() == 'fp32'
    return fp32.cpu().double(), x1.cpu().double(), emu.cpu().double(), l32, lx1


def _check_ratios(what, x1, emu, base):
    xm, xr = R.maxrms(x1 - base)
    em, er = R.maxrms(emu - base)
    print('%s: max %.3e vs %.3e (%.3f), rms %.3e vs %.3e (%.3f)' % (what, xm, em, xm / em, xr, er, xr / er))
    assert em > 0 and xm <= 1.5 * em and xr <= 1.25 * er, (what, xm, em, xr, er)


@pytest.mark.parametrize('cin,c2,planes', [(64, 0, 128), (32, 64, 64)])
def test_eval_basic_block(pkg, dev, monkeypatch, cin, c2, planes):
    ops = pkg.ops
    torch.manual_seed(3)
    blk = pkg.archs.BasicBlock(cin + c2, planes).to(dev).eval()
    _perturb_stats(blk, 4)
    g = torch.Generator().manual_seed(18)
    xc = torch.randn(2, cin, 20, 40, generator=g) * 1.5 + 0.3
    x2c = torch.randn(2, c2, 20, 40, generator=g) if c2 else None
    x = ops.to_nhwc(xc.to(dev)); x2 = ops.to_nhwc(x2c.to(dev)) if c2 else None
    fp32, x1, emu, l32, lx1 = _three_paths(pkg, monkeypatch, lambda: blk(x, x2))
    assert len(l32) == len(lx1) == 3 and not any('x1' in l for l in l32)
    assert ['halo_k32_x1' in l for l in lx1] == [True, False, True] and lx1[1] == l32[1]      # conv1, the 1x1 shortcut, conv2
    assert torch.isfinite(x1).all()
    _check_ratios('block vs FP32', x1, emu, fp32)
    # against the fp64 block of the helpers, over the helper's own error against the unrounded fp64 block
    folded = tuple(t.cpu() for t in blk._folded())
    sc = blk.shortcut[0].weight.detach().cpu()
    exact, _ = R.block64(xc, x2c, folded, sc, rounded=False)
    helper, _ = R.block64(xc, x2c, folded, sc, rounded=True)
    _check_ratios('block vs fp64', x1, helper, exact)
    # the training branch never reads the setting
    blk.train()
    ops.PROFILE = []
    try:
        with torch.no_grad(), ops.infer_precision('bf16x1'):
            blk(x, x2)
        assert not any('x1' in p[0] for p in ops.PROFILE)
    finally:
        ops.PROFILE = None


@pytest.fixture(scope='module')
def generator(pkg, dev):
    torch.manual_seed(41)
    model = pkg.archs.UNet_R_SS_v2(3, 3, False).to(dev).eval()
    _perturb_stats(model, 6)
    return model


def test_generator(pkg, dev, monkeypatch, generator):
    ops, A = pkg.ops, pkg.aerial_image_segmentation_api
    model = generator
    xc = torch.randn(2, 3, 128, 128, generator=torch.Generator().manual_seed(7))
    x = xc.to(dev)
    # the test's own evaluation of the predicate, from the shapes every eval BasicBlock sees
    expect = [0]

    def count(m, args):
        xs = [a for a in args if a is not None]
        w = xs[0].shape[3]
        planes, s = m.conv1.out_channels, m.conv1.stride[0]
        if s == 1 and all(t.shape[1] % 32 == 0 for t in xs) and planes % 64 == 0 and w >= 17:
            expect[0] += 1
        if planes % 64 == 0 and (w - 1) // s + 1 >= 17:                      # conv2: planes -> planes at the block's output size
            expect[0] += 1
    hooks = [m.register_forward_pre_hook(count) for m in model.modules() if isinstance(m, pkg.archs.BasicBlock)]
    with torch.no_grad():
        plain = model(x).clone()
    for h in hooks:
        h.remove()
    assert expect[0] > 0
    fp32, x1, emu, l32, lx1 = _three_paths(pkg, monkeypatch, lambda: model(x))
    assert torch.equal(fp32, plain.cpu().double()) and not any('x1' in l for l in l32)
    assert sum('halo_k32_x1' in l for l in lx1) == expect[0], (sum('halo_k32_x1' in l for l in lx1), expect[0])
    assert len(l32) == len(lx1)
    for a, b in zip(l32, lx1):                                              # every other conv keeps its previous label
        assert a == b or 'halo_k32_x1' in b, (a, b)
    assert torch.isfinite(x1).all()
    _check_ratios('generator logits vs FP32', x1, emu, fp32)
    # the API: no argument and 'fp32' are the plain model bit for bit; 'bf16x1' is the X1 path
    want = ops.sigmoid(plain).cpu()
    ops.PROFILE = []
    try:
        assert torch.equal(A.infer_patches(model, xc, batch_size=2), want)
        assert torch.equal(A.infer_patches(model, xc, batch_size=2, precision='fp32'), want)
        assert not any('x1' in p[0] for p in ops.PROFILE)
    finally:
        ops.PROFILE = None
    with torch.no_grad(), ops.infer_precision('bf16x1'):
        want_x1 = ops.sigmoid(model(x)).cpu()
    assert torch.equal(A.infer_patches(model, xc, batch_size=2, precision='bf16x1'), want_x1)


@pytest.mark.parametrize('size', [32, 64])
def test_segment_image_precision(pkg, dev, generator, size):
    A = pkg.aerial_image_segmentation_api
    img = np.random.default_rng(21).integers(0, 256, (96, 96, 3), dtype=np.uint8)
    cfg = dict(patch_size=64, input_w=size, input_h=size, patch_overlap=0.5, num_classes=3)
    base = A.segment_image(generator, img, cfg, batch_size=4)
    same = A.segment_image(generator, img, cfg, batch_size=4, precision='fp32')
    assert all(np.array_equal(a, b) for a, b in zip(base, same))
    pkg.ops.PROFILE = []
    try:
        got = A.segment_image(generator, img, cfg, batch_size=4, precision='bf16x1')
        assert any('halo_k32_x1' in p[0] for p in pkg.ops.PROFILE)
    finally:
        pkg.ops.PROFILE = None
    assert len(got) == 3
    for m in got:
        assert m.dtype == np.uint8 and m.shape == (96, 96) and set(np.unique(m)) <= {0, 255}
    print('segment_image %d: %.4f %% of mask bytes differ between the precisions'
          % (size, 100 * np.mean([np.mean(a != b) for a, b in zip(base, got)])))
    with pytest.raises(ValueError):
        A.segment_image(generator, img, cfg, precision='bf16')
    with pytest.raises(ValueError):
        A.infer_patches(generator, np.zeros((1, 3, 32, 32), np.float32), precision='medium')
    assert pkg.ops.infer_precision_mode() == 'fp32'


def test_graph_capture_is_keyed_by_precision(pkg, dev, generator):
    A, ops = pkg.aerial_image_segmentation_api, pkg.ops
    xc = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(9))
    a = A.infer_patches(generator, xc, batch_size=2, graph=True, precision='fp32')
    b = A.infer_patches(generator, xc, batch_size=2, graph=True, precision='bf16x1')
    c = A.infer_patches(generator, xc, batch_size=2, graph=True, precision='fp32')
    eager = A.infer_patches(generator, xc, batch_size=2, precision='bf16x1')
    assert torch.equal(a, c)
    assert torch.equal(b, eager)
    assert not torch.equal(a, b)
    assert torch.equal(a, A.infer_patches(generator, xc, batch_size=2))
