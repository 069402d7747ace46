"""archs.BasicBlock over frozen batch norms (blocks._FrozenBasicBlockFn), the mixed composition route, and one G+D step with
batchnorm.freeze_batch_norm on both models, at 2 x 64^2.

Block level, geometries (N, Cin [+ C2], planes, H, W) = the stem with shortcut, the two-pointer decoder block, an identity-shortcut
block and one on the generic kernels; running statistics with |mean| / sigma up to ~10, gamma of both signs, one gamma = 0 channel.
* forward: bit-identical to the same block's eval() + no_grad forward, running statistics and num_batches_tracked untouched, whether
  the block itself is in train or eval mode;
* backward against the same graph in fp64 on the CPU with the HIP masks imposed.  Yardstick: the composition a user could write
  before this node existed, ops.conv2d(x, W s, beta - mean s, act, res) with the fold as differentiable torch ops.  For every gradient
  tensor T: max|T_frozen - T_64| <= 2 max|T_composed - T_64| + 2^-24 max|T_64| (2 = the project's standing margin between two
  fp32-class summation orders; the floor is one rounding of the largest element).

Measured on an MI355X, max error / max|T_64| as "frozen node | composition | stock PyTorch fp32 on the CPU (against fp64 on its own masks)":

    stem         conv1.weight 3.2e-7 | 3.2e-7 | 3.0e-7    bn1.weight 8.6e-7 | 8.8e-7 | 1.3e-7    bn1.bias 9.8e-7 | 9.8e-7 | 3.9e-7
                 conv2.weight 2.3e-7 | 2.3e-7 | 7.9e-7    bn2.weight 6.7e-8 | 1.5e-7 | 2.3e-7    bn2.bias 2.3e-8 | 2.3e-8 | 2.3e-7
                 shortcut     1.6e-7 | 1.6e-7 | 2.9e-7    x1         1.3e-7 | 1.3e-7 | 2.4e-7
    two-pointer  bn1.weight   6.5e-7 | 6.5e-7 | 1.3e-7    bn1.bias   6.0e-7 | 6.0e-7 | 2.4e-7    conv2.weight 3.1e-7 | 3.1e-7 | 8.7e-7
                 bn2.weight   5.8e-8 | 5.9e-8 | 3.0e-7    bn2.bias   2.9e-8 | 2.9e-8 | 2.1e-7    shortcut 2.8e-7 | 2.8e-7 | 4.8e-7
                 x1           3.2e-7 | 3.2e-7 | 2.3e-7    x2         2.6e-7 | 2.6e-7 | 2.0e-7
    identity     bn1.weight   9.1e-7 | 9.1e-7 | 4.8e-7    bn1.bias   8.5e-7 | 8.5e-7 | 3.4e-7    conv2.weight 4.4e-7 | 4.4e-7 | 7.4e-7
                 bn2.weight   1.1e-7 | 1.2e-7 | 2.1e-7    bn2.bias   3.5e-8 | 3.5e-8 | 3.0e-7    x1 1.0e-7 | 1.0e-7 | 5.3e-8
    generic      bn1.weight   9.3e-8 | 3.5e-8 | 9.3e-8    bn1.bias   4.5e-8 | 4.5e-8 | 2.8e-8    conv2.weight 2.2e-7 | 2.2e-7 | 1.6e-7
                 bn2.weight   9.6e-8 | 2.2e-8 | 3.3e-8    bn2.bias   2.9e-8 | 2.9e-8 | 1.1e-7    x1 4.9e-8 | 4.9e-8 | 4.1e-8

Through the fold dgamma carries the conditioning |mean| / sigma (bn1.weight: up to x7 over stock autograd here, in both routes).
One G+D step, both models frozen, per-tensor error against fp64 on the same piece: median 1.4e-7, p95 5.8e-6, max 1.2e-5 (the oracle's
fp32 CPU path, same measure: 2.4e-7 / 5.9e-6 / 2.8e-5).  The file's 10 tests take 8 s, 3.5 s of it the three oracle runs of the step test.

Generator / trainer: after freeze_batch_norm, G.train() leaves every batch norm in eval mode; one gan_step leaves every running
statistic and num_batches_tracked bit-identical and moves every conv weight; logits equal G.eval() + no_grad bit for bit; generator
and discriminator gradients against oracle.seg_gan_cpu in fp64 (batch norms in eval mode, the HIP activation / pool pattern imposed)
under GRAD_RTOL / GRAD_ATOL and the "median <= 4 x the fp32 CPU path's median" rule of tests/test_grad_parity_gpu.py."""
import inspect

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import test_grad_parity_gpu as gp
from test_grad_parity_gpu import GRAD_ATOL, GRAD_RTOL, LR

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
GEOMS = [(2, 3, 0, 64, 32, 32), (2, 64, 128, 64, 32, 32), (1, 64, 0, 64, 20, 36), (2, 8, 0, 8, 9, 7)]
IDS = ['stem', 'two-pointer', 'identity', 'generic']


def _seed_stats(bn, g):
    """Running statistics of a trained layer: |mean| / sigma up to ~10, gamma of both signs, one gamma = 0 channel."""
    c = bn.num_features
    with torch.no_grad():
        var = torch.rand(c, generator=g) * 3.95 + 0.05
        bn.running_var.copy_(var)
        bn.running_mean.copy_((torch.rand(c, generator=g) * 20 - 10) * var.sqrt())
        w = (torch.rand(c, generator=g) + 0.5) * torch.where(torch.rand(c, generator=g) < 0.25, -1.0, 1.0)
        w[c // 2] = 0.0
        bn.weight.copy_(w); bn.bias.copy_(torch.randn(c, generator=g) * 0.3)


def _make(pkg, dev, geom, seed=5):
    n, c1, c2, planes, h, w = geom
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    blk = pkg.archs.BasicBlock(c1 + c2, planes)
    _seed_stats(blk.bn1, g); _seed_stats(blk.bn2, g)
    # inputs of the size the running statistics describe: conv outputs land around the running mean in some channels, far in others
    x1 = torch.randn(n, c1, h, w, generator=g)
    x2 = torch.randn(n, c2, h, w, generator=g) if c2 else None
    dout = torch.randn(n, planes, h, w, generator=g)
    return blk.to(dev), x1, x2, dout


def _bits(a, b):
    a = a.detach().contiguous(); b = b.detach().contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _stats(blk):
    return [t.clone() for bn in (blk.bn1, blk.bn2) for t in (bn.running_mean, bn.running_var, bn.num_batches_tracked)]


def _same_stats(blk, before):
    return all(torch.equal(a, b) for a, b in zip(_stats(blk), before))


PNAMES = ['conv1.weight', 'bn1.weight', 'bn1.bias', 'conv2.weight', 'bn2.weight', 'bn2.bias', 'shortcut.0.weight']


def _params(blk):
    d = dict(blk.named_parameters())
    return [(k, d[k]) for k in PNAMES if k in d]


def _run_frozen(blk, dev, x1, x2, dout, train_mode=True, input_grad=True):
    blk.train(train_mode)
    blk.bn1.eval(); blk.bn2.eval()
    blk.zero_grad(set_to_none=True)
    a = x1.to(dev).requires_grad_(input_grad)
    b = x2.to(dev).requires_grad_(input_grad) if x2 is not None else None
    out = blk(a, b)
    out.backward(dout.to(dev))
    grads = {k: (p.grad.detach().clone() if p.grad is not None else None) for k, p in _params(blk)}
    grads['x1'] = a.grad
    if b is not None:
        grads['x2'] = b.grad
    return out.detach(), grads


def _run_composed(pkg, blk, dev, x1, x2, dout):
    """What a user could already write: the fold as differentiable torch element-wise ops around ops.conv2d."""
    ops = pkg.ops
    blk.zero_grad(set_to_none=True)
    a = x1.to(dev).requires_grad_(True)
    b = x2.to(dev).requires_grad_(True) if x2 is not None else None
    st = blk.conv1.stride[0]
    fold = []
    for conv, bn in ((blk.conv1, blk.bn1), (blk.conv2, blk.bn2)):
        s = bn.weight * torch.rsqrt(bn.running_var + bn.eps)
        fold += [(conv.weight * s.view(-1, 1, 1, 1)).contiguous(), (bn.bias - bn.running_mean * s).contiguous()]
    y1 = ops.conv2d(a, fold[0], fold[1], st, 1, act=1, x2=b)
    r = ops.conv2d(a, blk.shortcut[0].weight, None, st, 0, x2=b) if len(blk.shortcut) else a
    out = ops.conv2d(y1, fold[2], fold[3], 1, 1, act=1, res=r)
    out.backward(dout.to(dev))
    grads = {k: p.grad.detach().clone() for k, p in _params(blk)}
    grads['x1'] = a.grad
    if b is not None:
        grads['x2'] = b.grad
    return out.detach(), y1.detach(), grads


def _run_cpu(blk, x1, x2, dout, m1, m2, dtype, batch_bn1=False):
    """The same graph with stock torch ops on the CPU in `dtype`; m1 / m2 = imposed masks (None: the graph's own)."""
    P = {k: v.detach().cpu().to(dtype).requires_grad_(v.dtype.is_floating_point and k.endswith(('weight', 'bias')))
         for k, v in list(blk.named_parameters()) + list(blk.named_buffers())}
    a = x1.detach().clone().to(dtype).requires_grad_(True)
    b = x2.detach().clone().to(dtype).requires_grad_(True) if x2 is not None else None
    x = a if b is None else torch.cat([a, b], 1)
    z1 = F.conv2d(x, P['conv1.weight'], None, blk.conv1.stride[0], 1)
    z1 = F.batch_norm(z1, None if batch_bn1 else P['bn1.running_mean'], None if batch_bn1 else P['bn1.running_var'], P['bn1.weight'], P['bn1.bias'],
                      batch_bn1, 0.0, blk.bn1.eps)
    y1 = torch.where(m1, z1, torch.zeros_like(z1)) if m1 is not None else F.relu(z1)
    z2 = F.batch_norm(F.conv2d(y1, P['conv2.weight'], None, 1, 1), P['bn2.running_mean'], P['bn2.running_var'], P['bn2.weight'], P['bn2.bias'],
                      False, 0.0, blk.bn2.eps)
    z2 = z2 + (F.conv2d(x, P['shortcut.0.weight'], None, blk.conv1.stride[0], 0) if 'shortcut.0.weight' in P else x)
    out = torch.where(m2, z2, torch.zeros_like(z2)) if m2 is not None else F.relu(z2)
    out.backward(dout.to(dtype))
    grads = {k: P[k].grad for k in PNAMES if k in P}
    grads['x1'] = a.grad
    if b is not None:
        grads['x2'] = b.grad
    return out.detach(), (z1.detach() > 0), (z2.detach() > 0), grads


@pytest.mark.parametrize('geom', GEOMS, ids=IDS)
def test_frozen_block_forward_and_backward(pkg, dev, geom):
    blk, x1, x2, dout = _make(pkg, dev, geom)
    blk.eval()
    with torch.no_grad():
        out0 = blk(x1.to(dev), x2.to(dev) if x2 is not None else None)
    before = _stats(blk)
    runs = {}
    for mode in (True, False):
        assert blk.train(mode) is blk
        blk.bn1.eval(); blk.bn2.eval()
        assert blk._route() == 'frozen'
        out, runs[mode] = _run_frozen(blk, dev, x1, x2, dout, train_mode=mode)
        assert _bits(out, out0), 'frozen forward differs from eval() + no_grad (block training=%s)' % mode
        assert _same_stats(blk, before), 'a frozen block wrote a running statistic'
    # a whole block in eval() with autograd on yields the frozen route's gradients, bit for bit
    for k, v in runs[True].items():
        assert v is not None and _bits(v, runs[False][k]), k
    gf = runs[True]
    outc, y1, gc = _run_composed(pkg, blk, dev, x1, x2, dout)
    assert _bits(outc, out0)
    _, _, _, g64 = _run_cpu(blk, x1, x2, dout, (y1 > 0).cpu(), (out0 > 0).cpu(), torch.float64)
    _, _, _, g32 = _run_cpu(blk, x1, x2, dout, None, None, torch.float32)
    _, m1s, m2s, _ = _run_cpu(blk, x1, x2, dout, None, None, torch.float64)
    _, _, _, g64s = _run_cpu(blk, x1, x2, dout, m1s, m2s, torch.float64)             # stock fp32 against fp64 on ITS own piece
    bad = []
    for k in gf:
        ref = g64[k]
        top = ref.abs().max().item()
        ef = (gf[k].cpu().double() - ref).abs().max().item()
        ec = (gc[k].cpu().double() - ref).abs().max().item()
        es = (g32[k].double() - g64s[k]).abs().max().item()
        tops = g64s[k].abs().max().item()
        print('RATIO %-12s %-18s frozen %.3e  composed %.3e  stock fp32 CPU %.3e   (max error / max|T_64|)'
              % (IDS[GEOMS.index(geom)], k, ef / top if top else 0.0, ec / top if top else 0.0, es / tops if tops else 0.0))
        if not ef <= 2 * ec + U32 * top:
            bad.append((k, ef, ec, top))
    assert not bad, bad


@pytest.mark.parametrize('geom', [GEOMS[1], GEOMS[3]], ids=[IDS[1], IDS[3]])
def test_requires_grad_off_returns_none_and_keeps_the_other_bits(pkg, dev, geom):
    blk, x1, x2, dout = _make(pkg, dev, geom)
    _, full = _run_frozen(blk, dev, x1, x2, dout)
    for bn in (blk.bn1, blk.bn2):
        bn.weight.requires_grad_(False); bn.bias.requires_grad_(False)
    _, g = _run_frozen(blk, dev, x1, x2, dout)
    for k, v in g.items():
        if k.startswith('bn'):
            assert v is None, k
        else:
            assert _bits(v, full[k]), k
    _, g = _run_frozen(blk, dev, x1, x2, dout, input_grad=False)
    assert g['x1'] is None and g.get('x2') is None
    for k in ('conv1.weight', 'conv2.weight', 'shortcut.0.weight'):
        if k in g:
            assert _bits(g[k], full[k]), k


def test_mixed_block_only_bn2_frozen(pkg, dev):
    """bn1 on batch statistics, bn2 frozen: the unfused composition; bn1's running estimates move, bn2's do not."""
    geom = GEOMS[3]
    blk, x1, x2, dout = _make(pkg, dev, geom)
    blk.train(); blk.bn2.eval()
    assert blk._route() == 'mixed'
    before = _stats(blk)
    a = x1.to(dev).requires_grad_(True)
    caught = []
    h = blk.bn1.register_forward_hook(lambda *_: caught.append(1))                       # modules are parameter holders: never called
    y1_mask = []
    bna = pkg.ops.batch_norm_act
    pkg.ops.batch_norm_act = lambda x, bn, **kw: (lambda y: (y1_mask.append((y.detach() > 0).cpu()), y)[1])(bna(x, bn, **kw))
    try:
        out = blk(a)
    finally:
        pkg.ops.batch_norm_act = bna; h.remove()
    out.backward(dout.to(dev))
    after = _stats(blk)
    assert not torch.equal(after[0], before[0]) and after[2].item() == before[2].item() + 1
    assert all(torch.equal(x, y) for x, y in zip(after[3:], before[3:]))
    _, _, _, g64 = _run_cpu(blk, x1, None, dout, y1_mask[0], y1_mask[1], torch.float64, batch_bn1=True)
    got = {k: p.grad for k, p in _params(blk)}
    got['x1'] = a.grad
    for k, ref in g64.items():
        err = (got[k].cpu().double() - ref).abs().max().item()
        assert err <= GRAD_RTOL * ref.abs().max().item() + GRAD_ATOL, (k, err, ref.abs().max().item())


# ----------------------------------------------------------------------------- generator and trainer at 2 x 64^2
class _Capture(gp._Capture):
    """tests/test_grad_parity_gpu.py's capture, plus the eval-mode batch norm (ops.batch_norm_act applies its activation itself)."""

    def __enter__(self):
        super().__enter__()
        ops = self.pkg.ops
        bna0 = ops.batch_norm_act
        cap = self

        def bna(x, bn, res=None, act=0, **kw):
            y = bna0(x, bn, res=res, act=act, **kw)
            if act != 0 and not bn.training:
                cap.items.append(cap._nchw_mask(y))
            return y
        self._saved.append((ops, 'batch_norm_act', bna0))
        ops.batch_norm_act = bna
        return self


def _seed_model_stats(model, seed):
    g = torch.Generator().manual_seed(seed)
    for m in model.modules():
        if isinstance(m, nn.modules.batchnorm._BatchNorm):
            with torch.no_grad():
                m.running_var.copy_(torch.rand(m.num_features, generator=g) * 1.5 + 0.5)
                m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.3)


def _bn_state(model):
    return [t.detach().cpu().clone() for m in model.modules() if isinstance(m, nn.modules.batchnorm._BatchNorm)
            for t in (m.running_mean, m.running_var, m.num_batches_tracked)]


@pytest.fixture(scope='module')
def frozen_step(pkg, dev):
    from oracle import seg_gan_cpu as O
    inp, tgt = O.synthetic_batch(2, 64, 64)
    torch.manual_seed(41)
    G = pkg.models_seg_gan.Generator(dict(arch='UNet_R_SS_v2', num_classes=3, input_channels=3, deep_supervision=False))
    D = pkg.models_seg_gan.Discriminator(3, kernel_size=3, n_channels=64, n_blocks=8, fc_size=1024)
    _seed_model_stats(G, 1); _seed_model_stats(D, 2)
    G.to(dev); D.to(dev)
    nG = pkg.batchnorm.freeze_batch_norm(G); nD = pkg.batchnorm.freeze_batch_norm(D)
    G.train(); D.train()
    modes = [m.training for mod in (G, D) for m in mod.modules() if isinstance(m, nn.modules.batchnorm._BatchNorm)]
    state0 = _bn_state(G) + _bn_state(D)
    conv0 = {k: m.weight.detach().cpu().clone() for k, m in G.named_modules() if isinstance(m, nn.Conv2d)}
    G.eval()
    with torch.no_grad():
        logits_eval = G(inp.to(dev)).detach().cpu().clone()
    G.train()
    with _Capture(pkg) as cap0:
        logits_train = G(inp.to(dev)).detach().cpu().clone()
    og = torch.optim.Adam(G.parameters(), lr=LR); od = torch.optim.Adam(D.parameters(), lr=LR)
    with _Capture(pkg) as cap:
        pkg.train_seg_gan.gan_step(inp.to(dev), tgt.to(dev), G, D, pkg.losses.BCEDiceLoss(), nn.BCEWithLogitsLoss(), nn.MSELoss(), og, od, 3)
    torch.cuda.synchronize()
    grads = [p.grad.detach().cpu().clone() for p in list(G.parameters()) + list(D.parameters())]
    conv1 = {k: m.weight.detach().cpu().clone() for k, m in G.named_modules() if isinstance(m, nn.Conv2d)}
    return dict(O=O, inp=inp, tgt=tgt, G=G, D=D, nG=nG, nD=nD, modes=modes, state0=state0, state1=_bn_state(G) + _bn_state(D), conv0=conv0,
                conv1=conv1, logits_eval=logits_eval, logits_train=logits_train, items=cap.items, grads=grads)


def test_freeze_survives_train_and_a_step_writes_no_statistic(frozen_step):
    s = frozen_step
    assert s['nG'] > 0 and s['nD'] == 7 and len(s['modes']) == s['nG'] + s['nD'] and not any(s['modes'])
    assert all(torch.equal(a, b) for a, b in zip(s['state0'], s['state1'])), 'a frozen step wrote a running statistic'
    still = [k for k in s['conv0'] if torch.equal(s['conv0'][k], s['conv1'][k])]
    assert not still, 'conv weights that did not move: %s' % still


def test_frozen_train_mode_logits_are_the_eval_logits(frozen_step, pkg):
    s = frozen_step
    # no module of this architecture other than BasicBlock and the batch norms reads `training` in its forward
    for m in s['G'].modules():
        if isinstance(m, (pkg.archs.BasicBlock, nn.modules.batchnorm._BatchNorm)):
            continue
        assert not isinstance(m, (nn.Dropout, nn.Dropout2d))
        fwd = type(m).forward
        if fwd is not nn.Module.forward and not type(m).__module__.startswith('torch.nn'):
            assert 'training' not in inspect.getsource(fwd), type(m)
    assert _bits(s['logits_train'], s['logits_eval'])


def test_frozen_step_gradients_vs_fp64(frozen_step):
    s = frozen_step
    O = s['O']

    def oracle(pattern, dtype):
        G, D, _, _ = O.make_models()
        _seed_model_stats(G, 1); _seed_model_stats(D, 2)
        G.to(dtype); D.to(dtype)
        for m in list(G.modules()) + list(D.modules()):
            if isinstance(m, nn.modules.batchnorm._BatchNorm):
                m.eval()
        og = torch.optim.Adam(G.parameters(), lr=LR); od = torch.optim.Adam(D.parameters(), lr=LR)
        snaps = {}

        def record(tag):
            if tag == 'g_bwd':
                snaps['G'] = [p.grad.detach().clone() for p in G.parameters()]
            if tag == 'd_bwd':
                snaps['D'] = [p.grad.detach().clone() for p in D.parameters()]
        O.PATTERN = pattern
        try:
            O.gan_step(G, D, og, od, s['inp'].to(dtype), s['tgt'].to(dtype), record=record)
        finally:
            O.PATTERN = None
        assert all(not m.training for m in G.modules() if isinstance(m, nn.modules.batchnorm._BatchNorm))
        return snaps['G'] + snaps['D'], [k for k, _ in G.named_parameters()] + ['D.' + k for k, _ in D.named_parameters()]

    g64, names = oracle(O.ActivationPattern('impose', [t.clone() for t in s['items']]), torch.float64)
    assert len(g64) == len(s['grads'])
    rel = []
    for name, a, b in zip(names, s['grads'], g64):
        b = b.clamp(-0.8, 0.8)
        scale = b.abs().max().item()
        err = (a.double() - b).abs().max().item()
        rel.append(err / scale if scale > 1e-6 else 0.0)
        assert err <= GRAD_RTOL * scale + GRAD_ATOL, '%s: |g_hip - g_fp64| = %.3e at max|g| = %.3e' % (name, err, scale)
    rel = np.array(rel)
    print('frozen step, gradient error vs fp64 on the same piece: median %.2e  p95 %.2e  max %.2e' % (np.median(rel), np.quantile(rel, 0.95), rel.max()))
    rec = O.ActivationPattern('record')
    g_ref32, _ = oracle(rec, torch.float32)
    g64_ref, _ = oracle(O.ActivationPattern('impose', [
        (r[1] > 0) if r[0] == 'act' else (((r[2] // r[1].shape[3]) % 2) * 2 + (r[2] % r[1].shape[3]) % 2) for r in rec.items]), torch.float64)
    rel_ref = np.array([(a.double() - b).abs().max().item() / b.abs().max().item() if b.abs().max().item() > 1e-6 else 0.0
                        for a, b in zip(g_ref32, g64_ref)])
    print('reference fp32 CPU path, same measure:                 median %.2e  p95 %.2e  max %.2e' % (np.median(rel_ref), np.quantile(rel_ref, 0.95), rel_ref.max()))
    assert np.median(rel) <= 4 * np.median(rel_ref) + 1e-7
