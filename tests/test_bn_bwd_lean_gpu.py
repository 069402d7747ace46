"""The lean batch-norm backward (ops.BN_BWD_LEAN) against the sequence it replaces, bit for bit.

Every comparison is torch.equal between the lean form and the form behind SSG_BN_BWD_LEAN=0, in this process (tensors that hold a
planted NaN are compared as int32 bit patterns, which is stricter):

  * kernel level: ssg_bn_apply_mask_f32 against ssg_bn_apply_f32 (y) and against numpy.packbits(y > 0, bitorder='little') along
    the channels (mask); ssg_bn_bwd_reduce_mask_f32 / ssg_bn_bwd_apply_mask_f32 against the forms that read y (sums, dx, dres,
    dweight, dbias); ssg_bn_bwd_apply_sums_f32 with the mask, with y and with the recomputed mask against ssg_bn_bwd_apply_f32,
    and its sum(dx) against ssg_channel_sum_f32 of the dx it returned.  The pre-activation is planted with +0.0, -0.0, a denormal,
    +-inf and NaN at fixed positions: x = -0.0 and shift = -0.0 there, so that fma(x, scale, shift) + res is res itself.
  * module level: archs.BasicBlock with identity and with 1 x 1 shortcut, a small Discriminator (every ConvolutionalBlock is
    the one-node conv -> BN -> act; the stem's activation backward and bias gradient are one sweep), and one gan_step of that
    discriminator with a small generator from the same seed: every gradient, every parameter after the step, the six scalars.

Shapes (N, H, W, C), the smallest that reach each path of the kernels: one pixel; two channel quads per mask byte with a ragged
pixel count; 64 channels (16 quads: a 16 x 16 block); 264 channels (66 quads: two channel groups, the second ragged); channel
slices of wider buffers (ld > C, the lanes outside the slice must keep their bytes); and 17 x 256 x 256 pixels, more rows than
MAX_PARTS parts of 8 rows per thread cover.  (2, 5, 5, 12): the predicate refuses C % 8 != 0.

The issue asked for Discriminator(..., fc_size=16); the class (as the reference's) hard-codes fc2 = Linear(1024, 1), so any
fc_size but 1024 cannot run a forward.  The discriminator here is Discriminator(3, n_channels=8, n_blocks=8, fc_size=1024)."""
import ctypes as C

import numpy as np
import pytest
import torch

RELU, LRELU = 1, 2
SENT = 777.0
# (N, H, W, C, sliced)
KERNEL_CASES = [(1, 1, 1, 8, False), (2, 19, 17, 8, False), (1, 5, 3, 64, False), (2, 9, 7, 264, False), (3, 33, 31, 32, True),
                (17, 256, 256, 8, False)]
SPECIALS = [0.0, -0.0, 1e-40, float('inf'), float('-inf'), float('nan')]


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


class _Buf(object):
    """[P, C] fp32 (or uint8) operand: dense, or a channel slice at lane `off` of a [P, ld] buffer filled with a sentinel."""

    def __init__(self, P, c, dev, sliced, dtype=torch.float32, data=None):
        self.c = c
        if sliced:
            self.ld, self.off = (c + 16, 8) if dtype == torch.float32 else (c + 3, 1)
        else:
            self.ld, self.off = c, 0
        self.buf = torch.full((P, self.ld), 77 if dtype == torch.uint8 else SENT, dtype=dtype, device=dev)
        self.v = self.buf[:, self.off:self.off + c]
        if data is not None:
            self.v.copy_(data)

    def outside_untouched(self):
        s = 77 if self.buf.dtype == torch.uint8 else SENT
        return bool((self.buf[:, :self.off] == s).all().item() and (self.buf[:, self.off + self.c:] == s).all().item())


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.gpu
@pytest.mark.parametrize('act,slope', [(RELU, 0.0), (LRELU, 0.2)])
@pytest.mark.parametrize('n,h,w,c,sliced', KERNEL_CASES)
def test_kernels_against_the_forms_that_read_y(pkg, dev, n, h, w, c, sliced, act, slope):
    lib = pkg._lib
    call, sp = lib.call, lib.stream_ptr
    P = n * h * w
    assert call('ssg_bn_mask_ok', c, act) == 1
    g = torch.Generator(device=dev).manual_seed(1000 * c + P % 997)

    def rnd(*shape):
        return torch.randn(*shape, generator=g, device=dev)
    xd, rd, dyd = rnd(P, c), rnd(P, c), rnd(P, c)
    scale = rnd(c).abs() + 0.5
    shift = rnd(c)
    for k, v in enumerate(SPECIALS):                       # pre-activation = v exactly at (pixel, channel k)
        pix = (5 * k) % P
        shift[k] = -0.0
        xd[pix, k] = -0.0
        rd[pix, k] = v
    x, res, dy = _Buf(P, c, dev, sliced, data=xd), _Buf(P, c, dev, sliced, data=rd), _Buf(P, c, dev, sliced, data=dyd)

    # ---- forward: y of today's entry, mask = packbits(y > 0)
    y0, y1 = _Buf(P, c, dev, sliced), _Buf(P, c, dev, sliced)
    mask = _Buf(P, c // 8, dev, sliced, dtype=torch.uint8)
    call('ssg_bn_apply_f32', _p(x.v), P, c, x.ld, _p(scale), _p(shift), _p(res.v), res.ld, act, slope, _p(y0.v), y0.ld, sp())
    call('ssg_bn_apply_mask_f32', _p(x.v), P, c, x.ld, _p(scale), _p(shift), _p(res.v), res.ld, act, slope, _p(y1.v), y1.ld,
         _p(mask.v), mask.ld, sp())
    torch.cuda.synchronize()
    assert torch.equal(_bits(y1.v), _bits(y0.v))
    yh = y0.v.cpu().numpy()
    for k, v in enumerate(SPECIALS):
        pre = yh[(5 * k) % P, k]
        if k == 2:                                         # the denormal: not asserted to survive the adds (a flush-to-zero mode would
            continue                                       # turn it into +0.0 in both entries alike); the bit comparisons cover it
        exp = np.float32(v) if not v < 0 else (np.float32(0.0) if act == RELU else np.float32(v) * np.float32(slope))
        assert (np.isnan(pre) and np.isnan(exp)) or (pre == exp and np.signbit(pre) == np.signbit(exp)), (k, v, pre)
    with np.errstate(invalid='ignore'):
        want = np.packbits(yh > 0, axis=1, bitorder='little')
    assert np.array_equal(mask.v.cpu().numpy(), want)
    assert y1.outside_untouched() and mask.outside_untouched()

    # ---- backward: statistics rows as a forward would have left them (any finite values do: both forms read the same rows)
    mean = rnd(c) * 0.1
    invstd = rnd(c).abs() + 0.5
    weight = rnd(c)
    ws = torch.empty(max(call('ssg_bn_workspace_bytes', P, c), 16) // 8, dtype=torch.float64, device=dev)
    s0 = torch.full((2 * c + 1,), -1.0, dtype=torch.float64, device=dev); s1 = s0.clone()
    call('ssg_bn_bwd_reduce_f32', _p(x.v), _p(y0.v), _p(dy.v), P, c, x.ld, y0.ld, dy.ld, _p(mean), _p(invstd), None, None, act, slope,
         _p(s0), 0, _p(ws), sp())
    call('ssg_bn_bwd_reduce_mask_f32', _p(x.v), _p(mask.v), _p(dy.v), P, c, x.ld, mask.ld, dy.ld, _p(mean), _p(invstd), act, slope,
         _p(s1), 0, _p(ws), sp())
    torch.cuda.synchronize()
    assert torch.isfinite(s0[:2 * c]).all()
    assert torch.equal(s1, s0)

    def outs():
        return (_Buf(P, c, dev, sliced), _Buf(P, c, dev, sliced), torch.empty(c, device=dev), torch.empty(c, device=dev))
    dx0, dr0, dw0, db0 = outs()
    call('ssg_bn_bwd_apply_f32', _p(x.v), _p(y0.v), _p(dy.v), P, c, x.ld, y0.ld, dy.ld, _p(mean), _p(invstd), _p(weight), None, None,
         _p(s0), float(P), act, slope, _p(dx0.v), dx0.ld, _p(dr0.v), dr0.ld, _p(dw0), _p(db0), sp())
    dx1, dr1, dw1, db1 = outs()
    call('ssg_bn_bwd_apply_mask_f32', _p(x.v), _p(mask.v), _p(dy.v), P, c, x.ld, mask.ld, dy.ld, _p(mean), _p(invstd), _p(weight),
         _p(s0), float(P), act, slope, _p(dx1.v), dx1.ld, _p(dr1.v), dr1.ld, _p(dw1), _p(db1), sp())
    torch.cuda.synchronize()
    assert torch.isfinite(dx0.v).all() and torch.isfinite(dr0.v).all()
    for a, b in ((dx1.v, dx0.v), (dr1.v, dr0.v), (dw1, dw0), (db1, db0)):
        assert torch.equal(a, b)
    assert dx1.outside_untouched() and dr1.outside_untouched()

    # ---- the apply pass that carries sum(dx): mask source = the bits, y, or recomputed from x
    csum = torch.empty(c, device=dev)
    call('ssg_channel_sum_f32', _p(dx0.v), P, c, dx0.ld, _p(csum), _p(ws), sp())
    for src in ('mask', 'y'):
        dx2, dr2, dw2, db2 = outs()
        dxsum = torch.full((c,), -1.0, device=dev)
        call('ssg_bn_bwd_apply_sums_f32', _p(x.v), _p(y0.v) if src == 'y' else None, _p(mask.v) if src == 'mask' else None, _p(dy.v),
             P, c, x.ld, y0.ld, mask.ld, dy.ld, _p(mean), _p(invstd), _p(weight), None, None, _p(s0), float(P), act, slope,
             _p(dx2.v), dx2.ld, _p(dr2.v), dr2.ld, _p(dw2), _p(db2), _p(dxsum), _p(ws), sp())
        torch.cuda.synchronize()
        for a, b in ((dx2.v, dx0.v), (dr2.v, dr0.v), (dw2, dw0), (db2, db0), (dxsum, csum)):
            assert torch.equal(a, b), src
        assert dx2.outside_untouched() and dr2.outside_untouched()
    # no residual in the forward: both forms recompute the mask from x with (scale, shift); no dres
    s2 = torch.empty(2 * c + 1, dtype=torch.float64, device=dev)
    call('ssg_bn_bwd_reduce_f32', _p(x.v), None, _p(dy.v), P, c, x.ld, 0, dy.ld, _p(mean), _p(invstd), _p(scale), _p(shift), act, slope,
         _p(s2), 0, _p(ws), sp())
    dx3, _, dw3, db3 = outs()
    call('ssg_bn_bwd_apply_f32', _p(x.v), None, _p(dy.v), P, c, x.ld, 0, dy.ld, _p(mean), _p(invstd), _p(weight), _p(scale), _p(shift),
         _p(s2), float(P), act, slope, _p(dx3.v), dx3.ld, None, 0, _p(dw3), _p(db3), sp())
    call('ssg_channel_sum_f32', _p(dx3.v), P, c, dx3.ld, _p(csum), _p(ws), sp())
    dx4, _, dw4, db4 = outs()
    dxsum = torch.full((c,), -1.0, device=dev)
    call('ssg_bn_bwd_apply_sums_f32', _p(x.v), None, None, _p(dy.v), P, c, x.ld, 0, 0, dy.ld, _p(mean), _p(invstd), _p(weight),
         _p(scale), _p(shift), _p(s2), float(P), act, slope, _p(dx4.v), dx4.ld, None, 0, _p(dw4), _p(db4), _p(dxsum), _p(ws), sp())
    torch.cuda.synchronize()
    for a, b in ((dx4.v, dx3.v), (dw4, dw3), (db4, db3), (dxsum, csum)):
        assert torch.equal(a, b)
    assert dx4.outside_untouched()


@pytest.mark.gpu
def test_refused_shape_keeps_reading_y(pkg, dev, monkeypatch):
    """(2, 5, 5, 12): C % 8 != 0.  The predicate says no, the launchers return a status, and the node saves y as before."""
    lib, ops = pkg._lib, pkg.ops
    assert lib.call('ssg_bn_mask_ok', 12, RELU) == 0
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 12, 5, 5, generator=g).to(dev); r = torch.randn(2, 12, 5, 5, generator=g).to(dev)
    dy = torch.randn(2, 12, 5, 5, generator=g).to(dev)
    bn = torch.nn.BatchNorm2d(12).to(dev).train()
    state = {k: v.clone() for k, v in bn.state_dict().items()}
    seen = []
    real = ops._bn_bwd_impl

    def spy(*a, **k):
        seen.append(k.get('mask') is not None)
        return real(*a, **k)
    monkeypatch.setattr(ops, '_bn_bwd_impl', spy)
    got = {}
    for lean in (0, 2):
        monkeypatch.setattr(ops, 'BN_BWD_LEAN', lean)
        bn.load_state_dict(state); bn.zero_grad(set_to_none=True)
        xd = x.clone().requires_grad_(True); rr = r.clone().requires_grad_(True)
        y = ops.batch_norm_act(xd, bn, res=rr, act=RELU)
        y.backward(dy)
        got[lean] = [y.detach(), xd.grad, rr.grad, bn.weight.grad, bn.bias.grad]
    assert seen == [False, False]
    for a, b in zip(got[2], got[0]):
        assert torch.equal(a, b)


def _lean_and_old(pkg, monkeypatch, build, run):
    """run(build()) under BN_BWD_LEAN = 0 and = 2 from the same seed; returns {lean: (named tensors, masks seen in the backward)}."""
    ops = pkg.ops
    out = {}
    real = ops._bn_bwd_impl
    for lean in (0, 2):
        seen = []

        def spy(*a, _seen=seen, **k):
            _seen.append((k.get('mask') is not None, bool(k.get('want_dxsum'))))
            return real(*a, **k)
        monkeypatch.setattr(ops, '_bn_bwd_impl', spy)
        monkeypatch.setattr(pkg.blocks, '_bn_bwd_impl', spy)
        monkeypatch.setattr(ops, 'BN_BWD_LEAN', lean)
        torch.manual_seed(23)
        out[lean] = (run(build()), seen)
    monkeypatch.setattr(ops, '_bn_bwd_impl', real)
    monkeypatch.setattr(pkg.blocks, '_bn_bwd_impl', real)
    return out


def _assert_same(new, old):
    assert [k for k, _ in new] == [k for k, _ in old]
    for (k, a), (_, b) in zip(new, old):
        assert torch.isfinite(b).all(), k
        assert torch.equal(a, b), (k, (a - b).abs().max().item())


@pytest.mark.gpu
@pytest.mark.parametrize('cin,cout', [(64, 64), (32, 64)], ids=['identity', 'conv1x1'])
def test_basic_block_lean_equals_old(pkg, dev, monkeypatch, cin, cout):
    g = torch.Generator().manual_seed(5)
    x0 = torch.randn(2, cin, 19, 17, generator=g).to(dev); dy = torch.randn(2, cout, 19, 17, generator=g).to(dev)

    def build():
        return pkg.archs.BasicBlock(cin, cout).to(dev).train()

    def run(m):
        assert (len(m.shortcut) > 0) == (cin != cout)
        x = x0.clone().requires_grad_(True)
        y = m(x)
        y.backward(dy)
        return [('out', y.detach()), ('dx', x.grad)] + [(k, v.grad) for k, v in m.named_parameters()] + \
               [(k, v.clone()) for k, v in m.named_buffers() if v.dtype.is_floating_point]
    r = _lean_and_old(pkg, monkeypatch, build, run)
    assert [s[0] for s in r[0][1]] == [False, False] and [s[0] for s in r[2][1]] == [True, False]     # bn2 (residual), bn1
    _assert_same(r[2][0], r[0][0])


def _disc(pkg, dev):
    return pkg.models_seg_gan.Discriminator(3, n_channels=8, n_blocks=8, fc_size=1024).to(dev).train()


@pytest.mark.gpu
def test_discriminator_lean_equals_old(pkg, dev, monkeypatch):
    ops = pkg.ops
    g = torch.Generator().manual_seed(9)
    x0 = torch.randn(2, 3, 96, 96, generator=g).to(dev)
    sweeps = []

    def recording(name, real, idx):
        def f(*a, **k):
            if a[idx].shape[2] > 1:                        # an image; the two Linear layers run as [1, O, 1, N] and keep their passes
                sweeps.append(name)
            return real(*a, **k)
        return f
    monkeypatch.setattr(ops, '_frozen_bwd', recording('frozen', ops._frozen_bwd, 2))
    monkeypatch.setattr(ops, '_channel_sum', recording('sum', ops._channel_sum, 0))
    monkeypatch.setattr(ops, '_act_bwd', recording('act', ops._act_bwd, 0))

    def run(m):
        del sweeps[:]
        x = x0.clone().requires_grad_(True)
        y = m(x)
        y.sum().backward()
        return [('out', y.detach()), ('dx', x.grad)] + [(k, v.grad) for k, v in m.named_parameters()] + \
               [(k, v.clone()) for k, v in m.named_buffers() if v.dtype.is_floating_point] + [('sweeps', torch.tensor([len(sweeps)]))], list(sweeps)
    r = _lean_and_old(pkg, monkeypatch, lambda: _disc(pkg, dev), run)
    (old, old_sweeps), old_bn = r[0]
    (new, new_sweeps), new_bn = r[2]
    # old: the stem's _act_bwd + _channel_sum and one _channel_sum per conv in front of a batch norm; lean: one sweep, no pass for a sum
    assert sorted(old_sweeps) == ['act'] + ['sum'] * 8 and new_sweeps == ['frozen']
    assert old_bn == [(False, False)] * 7 and new_bn == [(False, True)] * 7
    _assert_same(new[:-1], old[:-1])


@pytest.mark.gpu
def test_gan_step_lean_equals_old(pkg, dev, monkeypatch):
    import torch.nn as nn
    S = pkg
    g = torch.Generator().manual_seed(13)
    inp = torch.rand(2, 3, 96, 96, generator=g).to(dev)
    tgt = (torch.rand(2, 3, 96, 96, generator=g) > 0.5).float().to(dev)

    def build():
        G = S.models_seg_gan.Generator(dict(arch='UNet_R_SS_v2', num_classes=3, input_channels=3, deep_supervision=False)).to(dev).train()
        return G, _disc(pkg, dev)

    def run(models):
        G, D = models
        og = torch.optim.Adam(G.parameters(), lr=2e-5); od = torch.optim.Adam(D.parameters(), lr=2e-5)
        scal = S.train_seg_gan.gan_step(inp, tgt, G, D, S.losses.BCEDiceLoss(), nn.BCEWithLogitsLoss(), nn.MSELoss(), og, od, 3)
        torch.cuda.synchronize()
        named = [('scalar%d' % i, s.detach().reshape(1).float()) for i, s in enumerate(scal)]
        for tag, m in (('G.', G), ('D.', D)):
            named += [(tag + k + '.grad', v.grad) for k, v in m.named_parameters() if v.grad is not None]
            named += [(tag + k, v.detach().clone()) for k, v in m.named_parameters()]
            named += [(tag + k, v.clone()) for k, v in m.named_buffers() if v.dtype.is_floating_point]
        return named
    r = _lean_and_old(pkg, monkeypatch, build, run)
    assert len(r[2][0]) > 6 and any(s[0] for s in r[2][1]) and any(s[1] for s in r[2][1]) and not any(s[0] or s[1] for s in r[0][1])
    _assert_same(r[2][0], r[0][0])
