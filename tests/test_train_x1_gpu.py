"""ops.train_precision('bf16x1'): archs.BasicBlock, train mode and frozen, through blocks._BasicBlockFn / _FrozenBasicBlockFn on the
one-term bf16 kernels; ops.conv2d_bf16x1_train; train_seg_gan.gan_step(precision=...).

Blocks (train_x1_ref.CASES: 2 x 64 -> 64 on 8 x 24 with the identity shortcut, 2 x (64 + 64) -> 128 on 6 x 33 with the 1x1
shortcut).  For every gradient (x1, x2, w1, w2, wsc, gamma and beta of both batch norms) and the output, the device's error against
the UNQUANTISED fp64 block must be at most 1.5 x (max) / 1.25 x (RMS) of the error of the QUANTISED fp64 block of
tests/train_x1_ref.py (which rounds exactly where the kernels do), both references under the device's own ReLU masks.  Where no
rounding site reaches a tensor (wsc, beta2: the reference statistic is exactly zero) the gate is the project's fp32-class one,
GRAD_RTOL max|T| + GRAD_ATOL of tests/test_grad_parity_gpu.py.  The comparison is against the reference, never against the code
under test; tests/test_train_x1_ref.py shows what the statistic can see.

Also: mode 'fp32' is bit-identical to no context at all; backward uses its forward's mode; kernel ids 70 / 71 / 72 label the routed
launches (ops.PROFILE) and the shortcut and a 16-pixel-wide block stay on the old ids; two gan_steps with precision='bf16x1'."""
import contextlib

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import train_x1_ref as tr
from bn_ref import bf16_rne

pytestmark = pytest.mark.gpu

GRAD_RTOL, GRAD_ATOL = 1e-4, 1e-7          # tests/test_grad_parity_gpu.py: an fp32-class gradient against fp64 on the same piece
U32 = 2.0 ** -24
X1_CONV = ('conv_halo_k32_x1_kernel<128>', 'conv_halo_k32_x1_kernel<64>')
X1_WGRAD = 'wgrad_k32_x1_kernel'
NAME_OF = dict(tr.PARAM_OF)


def _build(pkg, dev, case, mode, st=None):
    st0, x1, x2, dout = tr.make_case(case)
    st = st or st0
    n, c1, c2, planes, h, w = tr.CASES[case]
    blk = pkg.archs.BasicBlock(c1 + c2, planes)
    if 'shortcut.0.weight' in st and not len(blk.shortcut):
        blk.shortcut = nn.Sequential(nn.Conv2d(c1 + c2, planes, kernel_size=1, bias=False))
    sd = blk.state_dict(); sd.update({k: v.clone() for k, v in st.items()})
    blk.load_state_dict(sd)
    blk.to(dev).train()
    if mode == 'frozen':
        blk.bn1.eval(); blk.bn2.eval()
    assert blk._route() == mode
    return blk, x1, x2, dout


def _run(pkg, blk, dev, x1, x2, dout, precision=None, leave_before_backward=False):
    blk.zero_grad(set_to_none=True)
    a = x1.to(dev).requires_grad_(True)
    b = x2.to(dev).requires_grad_(True) if x2 is not None else None
    ctx = pkg.ops.train_precision(precision) if precision else contextlib.nullcontext()
    with ctx:
        out = blk(a, b)
        if not leave_before_backward:
            out.backward(dout.to(dev))
    if leave_before_backward:
        out.backward(dout.to(dev))
    torch.cuda.synchronize()
    P = dict(blk.named_parameters())
    got = {'out': out.detach().cpu(), 'x1': a.grad.cpu()}
    if b is not None:
        got['x2'] = b.grad.cpu()
    for k, pk in NAME_OF.items():
        if pk in P:
            got[k] = P[pk].grad.detach().cpu()
    return got


def _device_masks(pkg, blk, dev, mode, x1, x2, out):
    """(y1 > 0, out > 0) of the device run: y1 recomputed by the launches the node makes (same kernels, same operands, same bits)."""
    ops = pkg.ops
    a = x1.to(dev); b = x2.to(dev) if x2 is not None else None
    with torch.no_grad():
        if mode == 'frozen':
            wf1, bf1, _, _ = blk._folded()
            y1 = ops._conv_bf16x1_impl(a, wf1, bf1, 1, 0.0, x2=b)
        else:
            c1 = ops._conv_bf16x1_impl(a, blk.conv1.weight, None, 0, 0.0, x2=b)
            bn = blk.bn1
            y1, _, _ = ops._bn_fwd_impl(c1, bn.weight, bn.bias, bn.running_mean.clone(), bn.running_var.clone(), None, float(bn.eps),
                                        float(bn.momentum), 1, 0.0, getattr(bn, '_ssg_var_mode', 0), None, part=None)
    return (y1 > 0).cpu(), out > 0


def _labels(pkg, fn):
    pkg.ops.PROFILE = []
    try:
        r = fn()
        torch.cuda.synchronize()
        return [rec[0] for rec in pkg.ops.PROFILE], r
    finally:
        pkg.ops.PROFILE = None


def _same(a, b):
    return set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)


# ----------------------------------------------------------------------------- the block gate
@pytest.mark.parametrize('mode', ['train', 'frozen'])
@pytest.mark.parametrize('case', sorted(tr.CASES))
def test_block_gradients_against_the_quantised_reference(pkg, dev, case, mode):
    blk, x1, x2, dout = _build(pkg, dev, case, mode)
    got = _run(pkg, blk, dev, x1, x2, dout, 'bf16x1')
    masks = _device_masks(pkg, blk, dev, mode, x1, x2, got['out'])
    stat = tr.stats(case, mode, tr.ALL, masks)
    ref = tr.tensors(case, mode, frozenset(), masks)
    assert set(stat) == set(got)
    bad = []
    for k in sorted(stat):
        smax, srms, scale = stat[k]
        emax, erms = tr.maxrms(got[k].double() - ref[k])
        floor = GRAD_RTOL * scale + GRAD_ATOL
        print('RATIO %-7s %-6s %-3s max %.3e / %.3e = %.3f   rms %.3e / %.3e = %.3f' % (
            case, mode, k, emax, smax, emax / smax if smax else float('nan'), erms, srms, erms / srms if srms else float('nan')))
        if not (emax <= max(tr.MAX_MARGIN * smax, floor) and erms <= max(tr.RMS_MARGIN * srms, floor)):
            bad.append((k, emax, smax, erms, srms))
    assert not bad, bad


# ----------------------------------------------------------------------------- modes
@pytest.mark.parametrize('mode', ['train', 'frozen'])
def test_mode_fp32_is_bit_identical_to_no_context(pkg, dev, mode):
    runs = []
    for precision in (None, 'fp32'):
        blk, x1, x2, dout = _build(pkg, dev, 'cat128', mode)
        labels, got = _labels(pkg, lambda: _run(pkg, blk, dev, x1, x2, dout, precision))
        runs.append((labels, got))
    assert runs[0][0] == runs[1][0], 'mode fp32 launches other kernels than no context'
    assert not any(l in X1_CONV or l == X1_WGRAD for l in runs[0][0])
    assert _same(runs[0][1], runs[1][1])
    blk, x1, x2, dout = _build(pkg, dev, 'cat128', mode)
    assert not _same(runs[0][1], _run(pkg, blk, dev, x1, x2, dout, 'bf16x1'))


@pytest.mark.parametrize('mode', ['train', 'frozen'])
def test_backward_uses_the_mode_of_its_forward(pkg, dev, mode):
    blk, x1, x2, dout = _build(pkg, dev, 'cat128', mode)
    inside = _run(pkg, blk, dev, x1, x2, dout, 'bf16x1')
    blk, x1, x2, dout = _build(pkg, dev, 'cat128', mode)
    labels, left = _labels(pkg, lambda: _run(pkg, blk, dev, x1, x2, dout, 'bf16x1', leave_before_backward=True))
    assert labels.count(X1_WGRAD) == 2
    assert _same(inside, left)
    # and a forward outside the context is not converted by a context around backward
    blk, x1, x2, dout = _build(pkg, dev, 'cat128', mode)
    plain = _run(pkg, blk, dev, x1, x2, dout)
    blk, x1, x2, dout = _build(pkg, dev, 'cat128', mode)
    blk.zero_grad(set_to_none=True)
    a = x1.to(dev).requires_grad_(True); b = x2.to(dev).requires_grad_(True)
    out = blk(a, b)
    labels, _ = _labels(pkg, lambda: _backward_in(pkg, out, dout.to(dev)))
    assert not any(l in X1_CONV or l == X1_WGRAD for l in labels)
    assert torch.equal(a.grad.cpu(), plain['x1'])


def _backward_in(pkg, out, dout):
    with pkg.ops.train_precision('bf16x1'):
        out.backward(dout)


def test_train_precision_context(pkg):
    ops = pkg.ops
    assert ops.train_precision_mode() == 'fp32'
    with ops.train_precision('bf16x1'):
        assert ops.train_precision_mode() == 'bf16x1'
        with ops.train_precision('fp32'):
            assert ops.train_precision_mode() == 'fp32'
        assert ops.train_precision_mode() == 'bf16x1'
    assert ops.train_precision_mode() == 'fp32'
    with pytest.raises(ValueError):
        ops.train_precision('bf16')
    assert 'train_precision' not in ops.__all__ and 'conv2d_bf16x1_train' not in ops.__all__
    assert ops.infer_precision_mode() == 'fp32'


# ----------------------------------------------------------------------------- routing
@pytest.mark.parametrize('mode', ['train', 'frozen'])
def test_routing_labels(pkg, dev, mode):
    lib = pkg._lib
    # two-pointer block with the 1x1 shortcut: 2 forward convs, dy1, dx1 and dx2 on ids 70 / 71; both weight gradients on id 72;
    # the shortcut's forward, weight gradient and two input-gradient slices on the old ids
    blk, x1, x2, dout = _build(pkg, dev, 'cat128', mode)
    labels, _ = _labels(pkg, lambda: _run(pkg, blk, dev, x1, x2, dout, 'bf16x1'))
    assert sum(l in X1_CONV for l in labels) == 5, labels
    assert labels.count(X1_WGRAD) == 2, labels
    others = [l for l in labels if l not in X1_CONV and l != X1_WGRAD]
    assert len(others) == 4 and '?' not in others, labels
    assert pkg.ops._WGRAD_X1_LABELS == {72: X1_WGRAD} and set(pkg.ops._X1_LABELS) == {70, 71}
    # identity-shortcut block: everything routed
    blk, x1, x2, dout = _build(pkg, dev, 'id64', mode)
    labels, _ = _labels(pkg, lambda: _run(pkg, blk, dev, x1, x2, dout, 'bf16x1'))
    assert sum(l in X1_CONV for l in labels) == 4 and labels.count(X1_WGRAD) == 2 and len(labels) == 6, labels
    # a 16-pixel-wide block stays on today's kernels, bit for bit
    g = torch.Generator().manual_seed(9)
    x = torch.randn(2, 64, 8, 16, generator=g); d = torch.randn(2, 64, 8, 16, generator=g)
    runs = []
    for precision in (None, 'bf16x1'):
        torch.manual_seed(3)
        blk = pkg.archs.BasicBlock(64, 64).to(dev).train()
        if mode == 'frozen':
            blk.bn1.eval(); blk.bn2.eval()
        runs.append(_labels(pkg, lambda: _run(pkg, blk, dev, x, None, d, precision)))
    assert runs[0][0] == runs[1][0] and not any(l in X1_CONV or l == X1_WGRAD for l in runs[1][0])
    assert _same(runs[0][1], runs[1][1])


# ----------------------------------------------------------------------------- ops.conv2d_bf16x1_train
def _q(t):
    return torch.from_numpy(bf16_rne(t.detach().float().numpy()).astype(np.float64))


def test_conv2d_bf16x1_train_gradients(pkg, dev):
    ops = pkg.ops
    g = torch.Generator().manual_seed(23)
    n, c1, c2, co, h, w = 2, 64, 64, 128, 6, 33
    x = torch.randn(n, c1, h, w, generator=g); x2 = torch.randn(n, c2, h, w, generator=g)
    wt = torch.randn(co, c1 + c2, 3, 3, generator=g) / (3 * (c1 + c2) ** 0.5)
    bias = torch.randn(co, generator=g) * 0.2; res = torch.randn(n, co, h, w, generator=g); dout = torch.randn(n, co, h, w, generator=g)
    T = [t.to(dev).requires_grad_(True) for t in (x, x2, wt, bias, res)]
    labels, y = _labels(pkg, lambda: ops.conv2d_bf16x1_train(T[0], T[2], T[3], act=1, x2=T[1], res=T[4]))
    assert labels == [X1_CONV[0]]
    labels, _ = _labels(pkg, lambda: y.backward(dout.to(dev)))
    assert sorted(labels) == sorted([X1_CONV[1], X1_CONV[1], X1_WGRAD]), labels
    # the quantised reference in fp64, the device's ReLU mask imposed
    xin = torch.cat([x, x2], 1)
    z = F.conv2d(_q(xin), _q(wt), bias.double(), 1, 1) + res.double()
    zmag = F.conv2d(_q(xin).abs(), _q(wt).abs(), bias.double().abs(), 1, 1) + res.double().abs()
    mask = (y.detach() > 0).cpu()
    K = 9 * (c1 + c2) + 2
    yref = torch.where(mask, z, torch.zeros_like(z))
    assert ((y.detach().cpu().double() - yref).abs() <= (K + 2) * U32 * zmag + U32 * yref.abs()).all()
    dy = torch.where(mask, dout, torch.zeros_like(dout))
    assert torch.equal(T[4].grad.cpu(), dy)                               # the residual's gradient is the masked dout itself
    P = n * h * w
    db = dy.double().sum((0, 2, 3)); dbmag = dy.double().abs().sum((0, 2, 3))
    assert ((T[3].grad.cpu().double() - db).abs() <= (P + 2) * U32 * dbmag + U32 * db.abs()).all()
    dw = torch.nn.grad.conv2d_weight(_q(xin), wt.shape, _q(dy), padding=1)
    dwmag = torch.nn.grad.conv2d_weight(_q(xin).abs(), wt.shape, _q(dy).abs(), padding=1)
    assert ((T[2].grad.cpu().double() - dw).abs() <= (P + 2) * U32 * dwmag + U32 * dw.abs()).all()
    dx = torch.nn.grad.conv2d_input(xin.shape, _q(wt), _q(dy), padding=1)
    dxmag = torch.nn.grad.conv2d_input(xin.shape, _q(wt).abs(), _q(dy).abs(), padding=1)
    gotx = torch.cat([T[0].grad.cpu(), T[1].grad.cpu()], 1).double()
    assert ((gotx - dx).abs() <= (9 * co + 2) * U32 * dxmag + U32 * dx.abs()).all()
    # refusals
    with pytest.raises(ValueError):
        ops.conv2d_bf16x1_train(torch.randn(1, 64, 8, 16, device=dev), T[2][:, :64])
    with pytest.raises(RuntimeError):
        ops.conv2d_bf16x1(T[0], T[2], x2=T[1])                             # the inference entry point still refuses a graph


# ----------------------------------------------------------------------------- gan_step
def _two_steps(pkg, dev, *extra, **kw):
    from oracle import seg_gan_cpu as O
    inp, tgt = O.synthetic_batch(2, 64, 64)
    torch.manual_seed(41)
    G = pkg.models_seg_gan.Generator(dict(arch='UNet_R_SS_v2', num_classes=3, input_channels=3, deep_supervision=False))
    D = pkg.models_seg_gan.Discriminator(3, 3, 64, 8, 1024)
    G.to(dev).train(); D.to(dev).train()
    p0 = [p.detach().cpu().clone() for p in G.parameters()]
    og = torch.optim.Adam(G.parameters(), lr=2e-5); od = torch.optim.Adam(D.parameters(), lr=2e-5)
    scal = []
    for _ in range(2):
        scal.append(pkg.train_seg_gan.gan_step(inp.to(dev), tgt.to(dev), G, D, pkg.losses.BCEDiceLoss(), nn.BCEWithLogitsLoss(), nn.MSELoss(),
                                               og, od, 3, *extra, **kw))
    torch.cuda.synchronize()
    return p0, [p.detach().cpu().clone() for p in list(G.parameters()) + list(D.parameters())], [[float(v) for v in s] for s in scal]


def test_gan_step_precision(pkg, dev):
    p0, base, s_base = _two_steps(pkg, dev)
    _, fp32, s_fp32 = _two_steps(pkg, dev, precision='fp32')
    assert s_base == s_fp32 and all(torch.equal(a, b) for a, b in zip(base, fp32)), "precision='fp32' differs from the positional-default call"
    labels, (_, x1, s_x1) = _labels(pkg, lambda: _two_steps(pkg, dev, precision='bf16x1'))
    assert len(s_x1) == 2 and all(len(s) == 6 and all(np.isfinite(v) for v in s) for s in s_x1), s_x1
    assert labels.count(X1_WGRAD) > 0 and sum(l in X1_CONV for l in labels) > 0
    ng = len(p0)
    assert all(not torch.equal(a, b) for a, b in zip(p0, x1[:ng]) if a.dim() == 4), 'a generator conv weight did not move'
    assert any(not torch.equal(a, b) for a, b in zip(base[:ng], x1[:ng])), 'the bf16x1 step equals the fp32 step'
    assert pkg.ops.train_precision_mode() == 'fp32'
