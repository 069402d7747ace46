"""What a training step does after the last conv, kernel by kernel against fp64 on the CPU: the fused loss / metric pass
(csrc/loss.hip), the discriminator BCE, clip + Adam and the weight / gradient clamps (csrc/pointwise.hip, optim.py) and the
spectral norm (csrc/spectral.hip).  The shapes are the smallest that leave each kernel's one-block, one-iteration path: a
subtle error here does not fault, it trains a slightly different model, and the step-level tests (six scalars at step
tolerances) would not see it.

Every reference is computed in fp64 from the same fp32 inputs -- the oracle's loss and metric functions on .double() tensors,
torch.optim.Adam on fp64 copies, an fp64 restatement of the power iteration -- never with the code under test."""
import copy
import math

import pytest
import torch
import torch.nn.functional as F

from test_ops_gpu import _close

pytestmark = pytest.mark.gpu


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _bits(t):
    return t.detach().contiguous().view(torch.int32).to('cpu', copy=True)


def _same(a, b):
    """torch.equal with NaN == NaN (torch.clamp and Adam both keep a NaN where it is)."""
    a = a.detach().cpu(); b = b.detach().cpu()
    return torch.equal(a.isnan(), b.isnan()) and torch.equal(torch.where(a.isnan(), torch.zeros_like(a), a),
                                                             torch.where(b.isnan(), torch.zeros_like(b), b))


# ============================================================================= seg_loss
SPECIAL_LOGITS = (30.0, -30.0, 88.0, -88.0, 100.0, -100.0, 0.0, -0.0)


def _seg_inputs(n, c, h, w, seed, special=False):
    """Logits randn * 3, targets in {0, 1}.  The hard IoU thresholds an fp32 sigmoid at 0.5 (as the reference project
    does), which an fp64 sigmoid contradicts for 0 < |x| < ~6e-8 by construction: no drawn logit is left inside
    (-1e-6, 1e-6).  The exact zeros of `special` are on the threshold in both precisions (sigmoid = 0.5, not > 0.5)."""
    g = _gen(seed)
    x = torch.randn(n, c, h, w, generator=g) * 3
    t = (torch.rand(n, c, h, w, generator=g) > 0.5).float()
    x[x.abs() < 1e-6] = 1e-3
    if special:
        flat = x.view(-1)
        pos = torch.randperm(flat.numel(), generator=g)[:4 * len(SPECIAL_LOGITS)]
        flat[pos] = torch.tensor(SPECIAL_LOGITS).repeat(4)          # each value four times: against targets 0 and 1, in every channel
    return x, t


def _seg_reference(x, t, mc0):
    """fp64: the oracle's functions for the six scalars, autograd of res[0] + 0.3 res[1] + 0.7 res[2] for the gradient."""
    from oracle import seg_gan_cpu as O
    xr = x.double().requires_grad_(True); td = t.double()
    loss = O.bce_dice_loss(xr, td); mse = F.mse_loss(xr, td); bce = O.stable_bce(xr, td)
    (loss + 0.3 * mse + 0.7 * bce).backward()
    n = x.shape[0]
    p = torch.sigmoid(xr.detach()).view(n, -1)
    dice_term = 1 - ((2.0 * (p * td.view(n, -1)).sum(1) + 1e-5) / (p.sum(1) + td.view(n, -1).sum(1) + 1e-5)).sum() / n
    xm = xr.detach()[:, mc0:].clone(); tm = td[:, mc0:].clone()
    return dict(scalars=[loss.item(), mse.item(), bce.item(), dice_term.item(), float(O.iou_score(xm, tm)), float(O.dice_coef(xm, tm))],
                grad=xr.grad)


SCALAR_NAMES = ('bce_dice', 'mse', 'stable_bce', 'dice_term', 'iou', 'dice')


def _check_scalars(res, ref, what):
    res = res.detach().cpu().double()
    for k, name in enumerate(SCALAR_NAMES):
        tol = 1e-6 if name == 'iou' else 1e-5 * max(1.0, abs(ref[k]))
        err = abs(res[k].item() - ref[k])
        print('%s %s: got %.9g ref %.9g err %.3e (tol %.3e)' % (what, name, res[k].item(), ref[k], err, tol))
        assert err <= tol, '%s %s: %.9g vs fp64 %.9g, err %.3e > %.3e' % (what, name, res[k].item(), ref[k], err, tol)
    assert res[6].item() == 1.0, '%s: finite flag' % what


def _check_seg(pkg, dev, x, t, mc0, what):
    ref = _seg_reference(x, t, mc0)
    xd = x.to(dev).requires_grad_(True)
    res = pkg.ops.seg_loss(xd, t.to(dev), mc0)
    (res[0] + 0.3 * res[1] + 0.7 * res[2]).backward()
    _check_scalars(res, ref['scalars'], what)
    # the 1e-8 floor of test_seg_loss_vs_oracle belongs to its 4320 elements: the gradient carries 1/numel, at larger sizes
    # the floor exceeds the gradient itself
    atol = 1e-8 if x.numel() <= 4320 else 0.0
    _close(xd.grad, ref['grad'], 1e-4, atol, what + ' grad')
    return xd.grad


SEG_CASES = [
    # n, c, h, w, mc0
    (3, 3, 1, 1, 1),           # S = 1: one thread active
    (2, 1, 15, 17, 0),         # S = 255, C = 1, every channel is a metric channel
    (2, 2, 16, 16, 2),         # mc0 >= C: no metric channel, IoU and Dice are the bare 1e-5 / 1e-5 quotients
    (2, 3, 16, 16, 5),
    (1, 3, 257, 3, 1),         # S = 771: four blocks for one sample, the last one ragged
    (5, 4, 33, 50, 3),         # several blocks per sample, mc0 = C - 1
    (130, 2, 3, 5, 1),         # N > 64: third chunk of seg_loss_final_kernel, stats indexed past sample 64
    (16, 3, 128, 128, 1),      # the bench's N and C: bps = 64, ppb = 256
]


@pytest.mark.parametrize('case', SEG_CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_seg_loss_paths(pkg, dev, case):
    n, c, h, w, mc0 = case
    x, t = _seg_inputs(n, c, h, w, seed=100 + n + 7 * c + h)
    _check_seg(pkg, dev, x, t, mc0, 'seg_loss %s' % (case,))


def test_seg_loss_extreme_logits(pkg, dev):
    """sigmoidf_(-100) goes through 1 / (1 + inf), logf(1 + expf(-|x|)) is not log1p: +-30, +-88, +-100 and both zeros.
    Found with this test: at a logit of exactly 0 autograd of the reference's clamp(x, 0) - x t + log(1 + exp(-|x|)) gives
    1 - t (clamp passes the gradient at x >= 0, |x| has slope 0), seg_loss_bwd_kernel gave sigmoid(0) - t = 0.5 - t, off by
    (0.5 g_seg + g_bce) / 2 numel = 3.9e-4 here against a bound of 4e-6.  The kernel now takes 1 - t at x == 0."""
    x, t = _seg_inputs(2, 3, 16, 16, seed=21, special=True)
    for v in SPECIAL_LOGITS:
        assert (x == v).sum() >= (8 if v == 0.0 else 4)
    grad = _check_seg(pkg, dev, x, t, 1, 'seg_loss extreme logits')
    assert torch.isfinite(grad).all()


def test_seg_loss_fp64_flush(pkg, dev):
    """The `cnt == 64` flush of a thread's fp32 partials into fp64 needs a block that owns >= 16384 pixels: N = 2048 samples
    of 128 x 128 one-channel pixels (bps = 1, ppb = 16384, every thread sees exactly 64 pixels), through the C ABI with
    ldx = ldt = 1 so that each input stays at 134 MB.  Forward only.
    Per-sample stats (sum p*t, sum p, sum t) at rtol 1e-6: 64 fp32 adds of positive terms per flush, 64 * 2^-24 ~ 4e-6 in
    the worst case and far less once 256 threads' independent roundings meet in fp64.
    Observed on an MI355X: largest relative error of the 6144 stats 2.4e-08."""
    from oracle import seg_gan_cpu as O
    n, s = 2048, 128 * 128
    g = _gen(22)
    x = torch.randn(n * s, generator=g) * 3
    t = (torch.rand(n * s, generator=g) > 0.5).float()
    x[x.abs() < 1e-6] = 1e-3
    L = pkg._lib
    assert L.call('ssg_seg_loss_workspace_bytes', n, s, 1) == n * 10 * 8       # one block per sample
    xd = x.to(dev); td = t.to(dev)
    res = torch.empty(8, dtype=torch.float32, device=dev)
    stats = torch.empty(3 * n + 5, dtype=torch.float64, device=dev)
    ws = torch.empty(L.call('ssg_seg_loss_workspace_bytes', n, s, 1) // 8, dtype=torch.float64, device=dev)
    L.call('ssg_seg_loss_fwd_f32', L.ptr(xd), 1, L.ptr(td), 1, n, s, 1, 0, L.ptr(res), L.ptr(stats), L.ptr(ws), L.stream_ptr())
    x4 = x.double().view(n, 1, 128, 128); t4 = t.double().view(n, 1, 128, 128)
    p = torch.sigmoid(x4).view(n, -1); tt = t4.view(n, -1)
    ref_stats = torch.stack([(p * tt).sum(1), p.sum(1), tt.sum(1)], 1)
    dice_n = (2.0 * ref_stats[:, 0] + 1e-5) / (ref_stats[:, 1] + ref_stats[:, 2] + 1e-5)
    dice_term = (1 - dice_n.sum() / n).item()
    bce = O.stable_bce(x4, t4).item()
    ref = [0.5 * bce + dice_term, F.mse_loss(x4, t4).item(), bce, dice_term, float(O.iou_score(x4, t4)), float(O.dice_coef(x4, t4))]
    _check_scalars(res, ref, 'seg_loss flush')
    got = stats[:3 * n].cpu().view(n, 3)
    rel = ((got - ref_stats).abs() / ref_stats.abs()).max().item()
    print('seg_loss flush: largest relative error of the per-sample stats %.3e' % rel)
    assert rel <= 1e-6, 'per-sample stats: relative error %.3e' % rel


def test_seg_loss_cross_rank_sums(pkg, dev):
    """The fp64[5] metric sums that the data-parallel path all-reduces: the halves of a batch add up to the whole batch's
    (the same fp64 block partials regrouped: S = 2000 gives 8 blocks per sample for N = 3 and N = 6 alike), and IoU / Dice
    rebuilt from the added sums are the whole batch's."""
    x, t = _seg_inputs(6, 3, 40, 50, seed=23)
    xd = x.to(dev); td = t.to(dev)
    res, sums = pkg.ops.seg_loss(xd, td, 1, with_sums=True)
    _, s_a = pkg.ops.seg_loss(xd[:3].contiguous(), td[:3].contiguous(), 1, with_sums=True)
    _, s_b = pkg.ops.seg_loss(xd[3:].contiguous(), td[3:].contiguous(), 1, with_sums=True)
    assert sums.dtype == torch.float64 and tuple(sums.shape) == (5,)
    added = (s_a + s_b).cpu(); full = sums.cpu()
    assert ((added - full).abs() <= 1e-12 * full.abs()).all(), (added, full)
    iou = (added[0] + 1e-5) / (added[1] + 1e-5)
    dice = (2 * added[2] + 1e-5) / (added[3] + added[4] + 1e-5)
    assert abs(iou.item() - res[4].item()) <= 1e-6 and abs(dice.item() - res[5].item()) <= 1e-6
    # and the sums themselves against fp64 (intersection and union are counts)
    p = torch.sigmoid(x.double())[:, 1:]; tm = t.double()[:, 1:]
    po = p > 0.5; to = tm > 0.5
    want = torch.stack([(po & to).sum().double(), (po | to).sum().double(), (p * tm).sum(), p.sum(), tm.sum()])
    assert full[0] == want[0] and full[1] == want[1]
    assert ((full[2:] - want[2:]).abs() <= 1e-6 * want[2:].abs()).all(), (full, want)


def test_seg_loss_reproducible(pkg, dev):
    """loss.hip sums in a fixed order: two runs of a multi-block shape agree bit for bit."""
    x, t = _seg_inputs(5, 4, 33, 50, seed=24)
    runs = []
    for _ in range(2):
        xd = x.to(dev).requires_grad_(True)
        res, stats = pkg.ops._SegLoss.apply(xd, t.to(dev), 3)
        (res[0] + 0.3 * res[1] + 0.7 * res[2]).backward()
        runs.append((res.detach().cpu(), stats.cpu(), xd.grad.cpu()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ============================================================================= bce_with_logits_const
@pytest.mark.parametrize('label', [0.0, 1.0, 0.9])
@pytest.mark.parametrize('n', [1, 255, 256, 257, 1000])
def test_bce_const_sizes_and_strides(pkg, dev, n, label):
    """Past one 256-stride of the forward loop and one block of the backward, on a dense [n, 1] tensor and on the
    [n, 1]-view-of-[n, 4] that the discriminator's linear layer hands over."""
    g = _gen(300 + n)
    x = torch.randn(n, 1, generator=g) * 4
    special = torch.tensor([100.0, -100.0, 0.0])[:n]
    x[torch.randperm(n, generator=g)[:len(special)], 0] = special
    xr = x.double().requires_grad_(True)
    lr = F.binary_cross_entropy_with_logits(xr, torch.full_like(xr, label)); lr.backward()
    canary = -7.25
    for strided in (False, True):
        if strided:
            buf = torch.full((n, 4), canary, device=dev)
            buf[:, 0] = x[:, 0].to(dev)
            xd = buf[:, :1].requires_grad_(True)
            assert xd.stride(0) == 4
        else:
            xd = x.to(dev).requires_grad_(True)
        ld = pkg.ops.bce_with_logits_const(xd, label); ld.backward()
        what = 'bce n=%d label=%g %s' % (n, label, 'strided' if strided else 'dense')
        err = abs(ld.item() - lr.item())
        assert err <= 1e-6 * max(1.0, abs(lr.item())), '%s: loss %.9g vs %.9g' % (what, ld.item(), lr.item())
        assert tuple(xd.grad.shape) == (n, 1)
        _close(xd.grad, xr.grad, 1e-5, 1e-7 * (4.0 / n if n > 4 else 1.0), what + ' grad')     # the gradient carries 1/n
        if strided:
            assert torch.equal(buf[:, 1:].cpu(), torch.full((n, 3), canary)) and torch.equal(buf[:, 0].cpu(), x[:, 0])


# ============================================================================= clip + Adam, clamps
ADAM_SIZES = (1, 3, 4, 5, 4095, 4096, 4097, 8192 + 6, 3 * 4096)
CANARY = -1.2345678e30
GAP = 8


class _Carved(object):
    """Views carved out of one flat device buffer, GAP-float canary gaps around them; every view starts `shift` floats
    past a 16-byte boundary."""

    def __init__(self, sizes, dev, shift=0):
        self.spans, off = [], GAP
        for n in sizes:
            start = (off + 3) // 4 * 4 + shift
            self.spans.append((start, n))
            off = start + n + GAP
        self.buf = torch.full((off,), CANARY, dtype=torch.float32, device=dev)
        assert self.buf.data_ptr() % 16 == 0
        self.gap = torch.ones(off, dtype=torch.bool)
        for start, n in self.spans:
            self.gap[start:start + n] = False
        self.views = [self.buf[start:start + n] for start, n in self.spans]
        for v in self.views:
            assert v.data_ptr() % 16 == 4 * shift
        self.canary_bits = _bits(torch.tensor([CANARY]))[0]

    def assert_gaps_intact(self, what):
        assert bool((_bits(self.buf)[self.gap] == self.canary_bits).all()), '%s: a canary gap was written' % what


def _adam_problem(dev, seed, shift_p=0, shift_g=0, sizes=ADAM_SIZES):
    """Device parameters (carved, with carved .grad) and their fp64 CPU twins."""
    g = _gen(seed)
    cp, cg = _Carved(sizes, dev, shift_p), _Carved(sizes, dev, shift_g)
    pd, pr = [], []
    for vp, vg in zip(cp.views, cg.views):
        val = torch.randn(vp.numel(), generator=g)
        vp.copy_(val); vg.zero_()
        p = vp.requires_grad_(True); p.grad = vg
        pd.append(p); pr.append(val.double().requires_grad_(True))
    return g, cp, cg, pd, pr


def _absmax(t):
    t = t.detach()[~t.detach().isnan()]
    return t.abs().max().item() if t.numel() else 0.0


def _param_tol(k, ref):
    # one fp32 rounding of the parameter per step, doubled for the roundings of m, v and the quotient (scaled down by lr <= 1e-2)
    return k * 2.0 ** -23 * max(1.0, _absmax(ref))


def _assert_near(got, ref, tol, what):
    got = got.detach().cpu().double(); ref = ref.detach()
    nan = ref.isnan()
    assert torch.equal(got.isnan(), nan), '%s: NaN positions differ' % what
    err = (got - ref)[~nan].abs().max().item() if (~nan).any() else 0.0
    assert err <= tol, '%s: max err %.3e > %.3e' % (what, err, tol)


def _set_grads(pd, pr, grads, clip):
    for p, r, gr in zip(pd, pr, grads):
        p.grad.copy_(gr)
        r.grad = (gr.clamp(-clip, clip) if clip else gr).double()


def _check_step(pkg, o_d, o_r, pd, pr, cp, cg, grads, clip, k, what):
    """One clip_adam_step against one fp64 step on the same fp32 gradients (clamped in fp32 first), then every bound; `k` is
    the number of steps the run takes."""
    _set_grads(pd, pr, grads, clip)
    o_r.step()
    pkg.optim.clip_adam_step(o_d, clip)
    cp.assert_gaps_intact(what + ' params'); cg.assert_gaps_intact(what + ' grads')
    # "their max" is the moment's largest magnitude over the optimizer's tensors, which one launch updates from gradients of
    # one scale.  Over a single tensor it is no bound on fp32 arithmetic: a 1-element exp_avg cancels to 0.4 % of the
    # gradients that went into it, and stock fp32 torch.optim.Adam is then 3.4 x outside k * 2^-22 of that value.
    scale = {key: max(_absmax(o_r.state[r][key]) for r in pr) for key in ('exp_avg', 'exp_avg_sq')}
    for i, (p, r, gr) in enumerate(zip(pd, pr, grads)):
        w = '%s tensor %d (n=%d)' % (what, i, p.numel())
        _assert_near(p, r, _param_tol(k, r), w + ' param')
        for key in ('exp_avg', 'exp_avg_sq'):
            ref = o_r.state[r][key]
            _assert_near(o_d.state[p][key], ref, k * 2.0 ** -22 * scale[key], w + ' ' + key)
        assert _same(p.grad, gr.clamp(-clip, clip) if clip else gr), w + ' clamped grad'
        assert float(o_d.state[p]['step']) == float(o_r.state[r]['step'])


def _randn_grads(g, pd, scale=2.0):
    return [torch.randn(p.numel(), generator=g) * scale for p in pd]


def _run_adam(pkg, dev, hyper, shift_p=0, shift_g=0, steps=5, seed=40):
    lr, betas, eps, wd, clip = hyper
    g, cp, cg, pd, pr = _adam_problem(dev, seed, shift_p, shift_g)
    kw = dict(lr=lr, betas=betas, eps=eps, weight_decay=wd)
    o_d = torch.optim.Adam(pd, **kw); o_r = torch.optim.Adam(pr, **kw)
    for it in range(steps):
        _check_step(pkg, o_d, o_r, pd, pr, cp, cg, _randn_grads(g, pd), clip, steps, 'adam %s step %d' % (hyper, it + 1))
    return [(_bits(p), _bits(o_d.state[p]['exp_avg']), _bits(o_d.state[p]['exp_avg_sq']), _bits(p.grad)) for p in pd]


ADAM_HYPER = [
    # lr, betas, eps, weight_decay, clip
    (1e-3, (0.9, 0.999), 1e-8, 0, 0.8),          # Adam's defaults
    (2e-4, (0.5, 0.999), 1e-8, 0, 0.8),          # the GAN betas
    (1e-2, (0.9, 0.99), 1e-3, 1e-2, None),
    (2e-3, (0.9, 0.999), 1e-8, 1e-2, 0.5),
]


@pytest.mark.parametrize('hyper', ADAM_HYPER, ids=lambda h: 'lr%g-b%g-eps%g-wd%g-clip%s' % (h[0], h[1][0], h[2], h[3], h[4]))
def test_clip_adam_hyperparameters(pkg, dev, hyper):
    _run_adam(pkg, dev, hyper)


@pytest.mark.parametrize('which', ['params', 'grads'])
def test_clip_adam_unaligned_is_bit_equal(pkg, dev, which):
    """Parameters (or gradients) 4 bytes off a 16-byte boundary take clamp_adam_kernel's scalar branch: the same function
    per element, so the same bits as the float4 branch on the same values.
    Found with this test: they were not the same bits.  The compiler contracted adam_elem differently in each inlined copy
    (float4 body: m + round(omb1 (g - m)) and fma(b2, v, .); scalar loop and n & 3 tail: fma(omb1, g - m, m) and
    round(b2 v) + .), so exp_avg and exp_avg_sq differed by an ulp.  adam_elem now spells its roundings out, in the float4
    body's form."""
    hyper = ADAM_HYPER[3]
    aligned = _run_adam(pkg, dev, hyper)
    shifted = _run_adam(pkg, dev, hyper, shift_p=int(which == 'params'), shift_g=int(which == 'grads'))
    for i, (a, b) in enumerate(zip(aligned, shifted)):
        for x, y, name in zip(a, b, ('param', 'exp_avg', 'exp_avg_sq', 'grad')):
            assert torch.equal(x, y), 'tensor %d %s differs between the float4 and the scalar branch' % (i, name)


def test_clip_adam_groups_and_missing_grad(pkg, dev):
    """Two parameter groups with their own lr and weight decay, and one parameter without a gradient: bit-unchanged, no state."""
    g, cp, cg, pd, pr = _adam_problem(dev, 41, sizes=ADAM_SIZES + (777,))
    idle_d, idle_r = pd.pop(), pr.pop()
    idle_d.grad = None
    before = _bits(idle_d)

    def groups(ps, idle):
        return [dict(params=ps[:4] + [idle], lr=1e-3, weight_decay=0.0), dict(params=ps[4:], lr=5e-3, weight_decay=1e-2)]
    o_d = torch.optim.Adam(groups(pd, idle_d), betas=(0.5, 0.999)); o_r = torch.optim.Adam(groups(pr, idle_r), betas=(0.5, 0.999))
    for it in range(5):
        _check_step(pkg, o_d, o_r, pd, pr, cp, cg, _randn_grads(g, pd), 0.8, 5, 'adam groups step %d' % (it + 1))
    assert torch.equal(_bits(idle_d), before) and idle_d.grad is None
    assert idle_d not in o_d.state or len(o_d.state[idle_d]) == 0


def test_clip_adam_resumed_state(pkg, dev):
    """A loaded state_dict with step = 1000 (bias corrections near 1) and non-zero moments; afterwards the device
    optimizer's state_dict loads into a stock CPU fp32 Adam whose next step() is the fp64 reference's next step."""
    hyper = ADAM_HYPER[3]
    lr, betas, eps, wd, clip = hyper
    kw = dict(lr=lr, betas=betas, eps=eps, weight_decay=wd)
    g, cp, cg, pd, pr = _adam_problem(dev, 42)
    o_d = torch.optim.Adam(pd, **kw); o_r = torch.optim.Adam(pr, **kw)
    moments = [(torch.randn(p.numel(), generator=g) * 0.1, torch.rand(p.numel(), generator=g) * 0.04 + 1e-4) for p in pd]

    def resumed(opt):
        state = {i: dict(step=torch.tensor(1000.0), exp_avg=m.clone(), exp_avg_sq=v.clone()) for i, (m, v) in enumerate(moments)}
        return dict(state=state, param_groups=opt.state_dict()['param_groups'])
    o_d.load_state_dict(resumed(o_d)); o_r.load_state_dict(resumed(o_r))
    assert o_d.state[pd[0]]['exp_avg'].device == pd[0].device and o_r.state[pr[0]]['exp_avg'].dtype == torch.float64
    for it in range(2):
        _check_step(pkg, o_d, o_r, pd, pr, cp, cg, _randn_grads(g, pd), clip, 2, 'adam resumed step %d' % (it + 1))
    assert float(o_d.state[pd[0]]['step']) == 1002.0
    pc = [p.detach().cpu().clone().requires_grad_(True) for p in pd]
    o_c = torch.optim.Adam(pc, **kw)
    o_c.load_state_dict(copy.deepcopy(o_d.state_dict()))
    assert float(o_c.state[pc[0]]['step']) == 1002.0 and o_c.state[pc[0]]['exp_avg'].device.type == 'cpu'
    grads = _randn_grads(g, pd)
    for c, r, gr in zip(pc, pr, grads):
        c.grad = gr.clamp(-clip, clip); r.grad = c.grad.double()
    o_c.step(); o_r.step()
    for i, (c, r) in enumerate(zip(pc, pr)):
        _assert_near(c, r, _param_tol(3, r), 'stock step after the device state_dict, tensor %d' % i)


def _with_specials(grads, values):
    """`values` at seeded positions of every tensor (cycled; a 1-element tensor gets the first)."""
    g = _gen(43)
    for gr in grads:
        pos = torch.randperm(gr.numel(), generator=g)[:len(values)]
        gr[pos] = torch.tensor(values)[:len(pos)]
    return grads


def test_clip_adam_special_gradients(pkg, dev):
    hyper = ADAM_HYPER[0]
    lr, betas, eps, wd, clip = hyper
    kw = dict(lr=lr, betas=betas, eps=eps, weight_decay=wd)
    inf = float('inf')
    # exactly +-clip and +-inf under a clip: clipped, finite
    g, cp, cg, pd, pr = _adam_problem(dev, 44)
    o_d = torch.optim.Adam(pd, **kw); o_r = torch.optim.Adam(pr, **kw)
    for it in range(2):
        grads = _with_specials(_randn_grads(g, pd), [inf, -inf, clip, -clip])
        _check_step(pkg, o_d, o_r, pd, pr, cp, cg, grads, clip, 2, 'adam +-clip, +-inf step %d' % (it + 1))
    for p in pd:
        assert all(torch.isfinite(t).all() for t in (p, p.grad, o_d.state[p]['exp_avg'], o_d.state[p]['exp_avg_sq']))
    # all-zero gradients: v stays 0, the parameter does not move
    g, cp, cg, pd, pr = _adam_problem(dev, 45)
    o_d = torch.optim.Adam(pd, **kw); o_r = torch.optim.Adam(pr, **kw)
    before = [_bits(p) for p in pd]
    for it in range(2):
        _check_step(pkg, o_d, o_r, pd, pr, cp, cg, [torch.zeros(p.numel()) for p in pd], clip, 2, 'adam zero grads step %d' % (it + 1))
    for p, b in zip(pd, before):
        assert torch.equal(_bits(p), b) and not o_d.state[p]['exp_avg_sq'].any() and not o_d.state[p]['exp_avg'].any()
    # one NaN per tensor, no clip: NaN at that position (as in torch), the neighbours within bound
    g, cp, cg, pd, pr = _adam_problem(dev, 46)
    o_d = torch.optim.Adam(pd, **kw); o_r = torch.optim.Adam(pr, **kw)
    grads = _with_specials(_randn_grads(g, pd), [float('nan')])
    _check_step(pkg, o_d, o_r, pd, pr, cp, cg, grads, None, 2, 'adam NaN grad step 1')
    _check_step(pkg, o_d, o_r, pd, pr, cp, cg, _randn_grads(g, pd), None, 2, 'adam NaN grad step 2')
    for p, r in zip(pd, pr):
        assert int(p.isnan().sum()) == 1 and int(r.isnan().sum()) == 1


def test_weight_and_gradient_clamps(pkg, dev):
    """clamp_parameters_ and srgan_utils.clip_gradient are torch.clamp, NaN kept, nothing else touched."""
    inf, clip = float('inf'), 0.7
    g, cp, cg, pd, _ = _adam_problem(dev, 47)
    vals = _with_specials([torch.randn(p.numel(), generator=g) * 2 for p in pd], [clip, -clip, inf, -inf, float('nan')])
    grads = _with_specials([torch.randn(p.numel(), generator=g) * 2 for p in pd], [float('nan'), -inf, inf, -clip, clip])
    for p, v, gr in zip(pd, vals, grads):
        p.detach().copy_(v); p.grad.copy_(gr)
    gbits = _bits(cg.buf)
    pkg.optim.clamp_parameters_(pd, clip)
    cp.assert_gaps_intact('clamp_parameters_')
    for i, (p, v) in enumerate(zip(pd, vals)):
        assert _same(p, v.clamp(-clip, clip)), 'clamp_parameters_ tensor %d' % i
    assert torch.equal(_bits(cg.buf), gbits), 'clamp_parameters_ touched a gradient'
    pbits = _bits(cp.buf)
    pkg.srgan_utils.clip_gradient(torch.optim.Adam(pd), 0.3)
    cg.assert_gaps_intact('clip_gradient')
    for i, (p, gr) in enumerate(zip(pd, grads)):
        assert _same(p.grad, gr.clamp(-0.3, 0.3)), 'clip_gradient tensor %d' % i
    assert torch.equal(_bits(cp.buf), pbits), 'clip_gradient touched a weight'


def test_clip_adam_recycled_addresses(pkg, dev):
    """A 5000-element parameter at the four addresses of an earlier 10000-element one (what the caching allocator hands a
    second model after the first was freed) gets a plan of its own: elements 5000.. of all four tensors stay as they were.
    The weight clamp likewise.  (Host side: test_host_logic.py::test_launch_plans_follow_sizes_at_recycled_addresses.)"""
    g = _gen(48)
    roles = [_Carved((10000,), dev) for _ in range(4)]               # param, grad, exp_avg, exp_avg_sq

    def optimizer(n):
        p, gr, m, v = [r.buf[r.spans[0][0]:r.spans[0][0] + n] for r in roles]
        p = p.requires_grad_(True); p.grad = gr
        opt = torch.optim.Adam([p], lr=1e-2)
        opt.state[p] = dict(step=torch.tensor(0.0), exp_avg=m, exp_avg_sq=v)
        return p, opt
    roles[0].views[0].copy_(torch.randn(10000, generator=g))
    roles[2].views[0].zero_(); roles[3].views[0].zero_()
    big, o_big = optimizer(10000)
    big.grad.copy_(torch.randn(10000, generator=g) * 2)
    pkg.optim.clip_adam_step(o_big, 0.8)
    pkg.optim.clamp_parameters_([big], 3.0)
    before = [_bits(r.buf) for r in roles]
    small, o_small = optimizer(5000)
    assert [t.data_ptr() for t in (small, small.grad, o_small.state[small]['exp_avg'], o_small.state[small]['exp_avg_sq'])] == \
           [t.data_ptr() for t in (big, big.grad, o_big.state[big]['exp_avg'], o_big.state[big]['exp_avg_sq'])]
    small.grad.copy_(torch.randn(5000, generator=g) * 2)
    pkg.optim.clip_adam_step(o_small, 0.8)
    pkg.optim.clamp_parameters_([small], 0.5)
    start = roles[0].spans[0][0]
    for r, b, name in zip(roles, before, ('param', 'grad', 'exp_avg', 'exp_avg_sq')):
        now = _bits(r.buf)
        assert torch.equal(now[start + 5000:], b[start + 5000:]), '%s written past the 5000-element tensor' % name
        assert not torch.equal(now[start:start + 5000], b[start:start + 5000]), '%s: the step did not run' % name
        r.assert_gaps_intact('recycled ' + name)
    assert small.detach().abs().max().item() <= 0.5 and big.detach()[5000:].abs().max().item() > 0.5


# ============================================================================= spectral norm
def _sn_reference(w, u, v, n_iter, dwsn, eps=1e-12):
    """spectral_norm.py:73-88 in fp64: the power iteration without gradient, sigma = u . (W v), W / sigma; dW by autograd."""
    wm = w.double().reshape(w.shape[0], -1).requires_grad_(True)
    u = u.double(); v = v.double()
    with torch.no_grad():
        for _ in range(n_iter):
            v = F.normalize(wm.t() @ u, dim=0, eps=eps)
            u = F.normalize(wm @ v, dim=0, eps=eps)
    sigma = torch.dot(u, wm @ v)
    wsn = wm / sigma
    wsn.backward(dwsn.double().reshape(wm.shape))
    return u, v, wsn.detach().reshape(w.shape), sigma.item(), wm.grad.reshape(w.shape)


SN_CASES = [
    # rows, cols
    (1, 300), (300, 1),        # u or v of length 1
    (64, 27),                  # the discriminator's first layer
    (257, 513),                # both 256-stride loops take a second, ragged pass
    (512, 4608),               # n = 2.36M: grid-stride in scale_kernel and sn_bwd_kernel, the 512-partial cap of the backward dot
]


@pytest.mark.parametrize('n_iter', [0, 1, 3])
@pytest.mark.parametrize('rows,cols', SN_CASES)
def test_spectral_norm_weight_paths(pkg, dev, rows, cols, n_iter):
    g = _gen(500 + rows + cols)
    shape = (rows, cols // 9, 3, 3) if cols % 9 == 0 else (rows, cols, 1, 1)
    w = torch.randn(shape, generator=g) / math.sqrt(cols)
    u = F.normalize(torch.randn(rows, generator=g), dim=0); v = F.normalize(torch.randn(cols, generator=g), dim=0)
    if n_iter == 0:
        # eval mode meets the vectors training left behind, not the random initial ones (whose u . W v is near 0)
        u, v = [t.float() for t in _sn_reference(w, u, v, 2, torch.zeros(shape))[:2]]
    dwsn = torch.randn(shape, generator=g)
    ur, vr, wr, sr, dwr = _sn_reference(w, u, v, n_iter, dwsn)
    assert sr > 0.5                                                            # sigma is O(1) by construction
    runs = []
    for _ in range(2):
        wd = w.to(dev).requires_grad_(True); ud = u.to(dev); vd = v.to(dev)
        out, sigma = pkg.ops.spectral_norm_weight(wd, ud, vd, n_iter)
        out.backward(dwsn.to(dev))
        runs.append([t.detach().cpu() for t in (ud, vd, out, sigma, wd.grad)])
    ud, vd, out, sigma, dw = runs[0]
    what = 'spectral norm %dx%d, %d iterations' % (rows, cols, n_iter)
    if n_iter == 0:
        assert torch.equal(_bits(ud), _bits(u)) and torch.equal(_bits(vd), _bits(v)), what + ': u, v moved'
    _close(ud, ur, 0, 2e-6, what + ' u'); _close(vd, vr, 0, 2e-6, what + ' v')
    _close(out, wr, 0, 2e-6 * max(1.0, wr.abs().max().item()), what + ' W / sigma')
    assert abs(sigma.item() - sr) <= 2e-6 * abs(sr), '%s sigma %.9g vs %.9g' % (what, sigma.item(), sr)
    _close(dw, dwr, 1e-4, 1e-6, what + ' dW')
    for a, b in zip(*runs):
        assert torch.equal(a, b), what + ': two identical calls differ'
