"""The lean SPADE backward (blocks._SpadeFn.backward where blocks._spade_bwd_route says so): d(beta) = dout is not copied, dx = dout*(1+gamma) is not stored.

  * all nine gradients of the node against an fp64 torch.autograd restatement on the CPU (out = x*(1+gamma(a)) + beta(a),
    a = relu(shared(x2map(x)))), with SSG_SPADE_BWD_LEAN's switch at 2 (lean wherever its kernels allow, whatever the size) and at 0 on the same inputs: per gradient, the lean path's
    max and rms error may be at most 2 x the old path's (the gate of tests/test_split_gpu.py, without its absolute slack);
  * ssg_spade_modulate_dgamma_sums_f32 against ssg_spade_modulate_bwd_sums_f32: d(gamma) and the 2C fp64 sums bit for bit;
  * ssg_spade_dgrad_modulate_f32 against the residual launch it replaces.  The epilogue forms fl(dout * fl(1 + gamma)) with
    the two operations the old modulate pass used and adds it as the residual launch adds res (include/ssunet_hip.h: no fused
    multiply-add), so the expectation is exact: dx carries the bits of old dgrad + dxm.  With that, seven of the nine gradients
    of the lean path equal the old path's (asserted too): everything but the weight gradients of the gamma and beta convs,
    whose two C-channel launches may split the pixel reduction differently from the one 2C-channel launch;
  * (no GPU) the per-layer router keeps the old sequence wherever a query declines.

Shapes: the smallest that reach each route -- 65536 pixels (threshold of the fused forward and of thin32_cin), an unfused level
(thin4_cin and the 4x4x1 thin-Cout kernel), a ragged one (19 x 17: a one-pixel 4-strip and a 3-row band of thin4_cin, a
partial 62-column strip of the thin-Cout rows form), and a 384-channel one whose two-pointer input gradient is an MFMA
kernel's; the kernel-level cases add a ragged 32-pixel strip of thin32_cin (W = 257) and channel counts that leave the second
32-channel fragment (96) and the last 64-channel group (40) partly empty."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

# N, C, H, W; nhidden = max(C / 16, 4), 3 classes.  The two-pointer input gradient of the gamma|beta conv runs on
# thin4_cout_kernel_rows (C = 64), thin4_cout_kernel (C = 128) and, in the fourth case (nhidden = 24), on an MFMA kernel.
CASES = [(1, 64, 256, 256), (2, 128, 24, 24), (1, 64, 19, 17), (1, 384, 9, 10)]
KERNEL_CASES = CASES[:3] + [(1, 96, 256, 257), (1, 40, 19, 17)]


def _reference(m, x, dy):
    """The nine gradients in fp64 on the CPU, keyed 'x' and by parameter name."""
    P = {k: v.detach().cpu().double().requires_grad_(True) for k, v in m.named_parameters()}
    xr = x.double().requires_grad_(True)
    seg = F.conv2d(xr, P['x2map.weight'], P['x2map.bias'], 1, 1)
    a = F.relu(F.conv2d(seg, P['mlp_shared.0.weight'], P['mlp_shared.0.bias'], 1, 1))
    gam = F.conv2d(a, P['mlp_gamma.weight'], P['mlp_gamma.bias'], 1, 1)
    bet = F.conv2d(a, P['mlp_beta.weight'], P['mlp_beta.bias'], 1, 1)
    (xr * (1 + gam) + bet).backward(dy.double())
    ref = {k: v.grad for k, v in P.items()}
    ref['x'] = xr.grad
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize('n,c,h,w', CASES)
def test_nine_gradients_against_fp64_lean_and_old(pkg, dev, monkeypatch, n, c, h, w):
    blocks = pkg.blocks
    torch.manual_seed(31)
    m = pkg.normalization.SPADE('spadebatch3x3', c, 3, c / 16).to(dev).train()
    g = torch.Generator().manual_seed(7)
    x = torch.randn(n, c, h, w, generator=g); dy = torch.randn(n, c, h, w, generator=g)
    ref = _reference(m, x, dy)
    assert len(ref) == 9
    routes = []
    real = blocks._spade_bwd_route

    def recording(*a, **k):
        routes.append(real(*a, **k))
        return routes[-1]
    monkeypatch.setattr(blocks, '_spade_bwd_route', recording)
    got = {}
    for lean in (0, 2):
        monkeypatch.setattr(blocks, 'SPADE_BWD_LEAN', lean)
        m.zero_grad(set_to_none=True)
        xd = x.to(dev).requires_grad_(True)
        m(xd, xd).backward(dy.to(dev))
        got[lean] = {k: v.grad.detach().cpu().double() for k, v in m.named_parameters()}
        got[lean]['x'] = xd.grad.detach().cpu().double()
    assert routes == [False, True], routes
    for k in sorted(ref):
        e_old = (got[0][k] - ref[k]).abs(); e_new = (got[2][k] - ref[k]).abs()
        mo, mn = e_old.max().item(), e_new.max().item()
        ro, rn = e_old.pow(2).mean().sqrt().item(), e_new.pow(2).mean().sqrt().item()
        print('%-22s max err old %.3e lean %.3e   rms old %.3e lean %.3e   (ref max %.3e)   %s'
              % (k, mo, mn, ro, rn, ref[k].abs().max().item(), 'same bits' if torch.equal(got[2][k], got[0][k]) else ''))
    for k in sorted(ref):
        e_old = (got[0][k] - ref[k]).abs(); e_new = (got[2][k] - ref[k]).abs()
        assert e_new.max().item() <= 2.0 * e_old.max().item(), (k, e_new.max().item(), e_old.max().item())
        assert e_new.pow(2).mean().sqrt().item() <= 2.0 * e_old.pow(2).mean().sqrt().item(), k
    # same products, same order of every reduction: the lean path gives the old path's bits, but for the two weight gradients
    # whose launches were split in two (their split-K partition follows the launch's own column tiles)
    for k in sorted(ref):
        if k not in ('mlp_gamma.weight', 'mlp_beta.weight'):
            assert torch.equal(got[2][k], got[0][k]), k


@pytest.mark.gpu
@pytest.mark.parametrize('n,c,h,w', KERNEL_CASES)
@pytest.mark.parametrize('gamma_only', [True, False])
def test_kernels_against_the_pair_they_replace(pkg, dev, n, c, h, w, gamma_only):
    ops, blocks = pkg.ops, pkg.blocks
    call, ptr, sp = pkg._lib.call, pkg._lib.ptr, pkg._lib.stream_ptr
    g = torch.Generator().manual_seed(11)

    def rnd(ch, ld=None):
        t = ops.new_nhwc(n, ch, h, w, dev, ld=ld, zero=True)
        t.copy_(torch.randn(n, ch, h, w, generator=g))
        return t
    x, dout, dseg = rnd(c), rnd(c), rnd(3)
    gb = rnd(c) if gamma_only else rnd(2 * c)            # gamma alone (fused forward) or gamma|beta rows (pixel stride 2C)
    wx = torch.randn(3, c, 3, 3, generator=g).to(dev)
    p = n * h * w
    ws = ops._ws(call('ssg_bn_workspace_bytes', p, c), dev)
    # the old pass
    dxm = ops.new_nhwc(n, c, h, w, dev); dgb = ops.new_nhwc(n, 2 * c, h, w, dev)
    sums_old = torch.empty(2 * c, dtype=torch.float64, device=dev)
    call('ssg_spade_modulate_bwd_sums_f32', ptr(x), ops._ld(x), ptr(gb), ops._ld(gb), ptr(dout), ops._ld(dout), p, c,
         ptr(dxm), ops._ld(dxm), ptr(dgb), ops._ld(dgb), ptr(sums_old), ptr(ws), sp())
    dx_old = ops._conv_dgrad_impl(dseg, wx, 1, 1, h, w, 0, c, res=dxm)
    # the lean pass
    dgamma = ops.new_nhwc(n, c, h, w, dev)
    sums_new = torch.empty(2 * c, dtype=torch.float64, device=dev)
    call('ssg_spade_modulate_dgamma_sums_f32', ptr(x), ops._ld(x), ptr(dout), ops._ld(dout), p, c, ptr(dgamma), ops._ld(dgamma),
         ptr(sums_new), ptr(ws), sp())
    assert torch.equal(dgamma, dgb[:, :c])
    assert torch.equal(dgb[:, c:], dout)
    assert torch.equal(sums_new, sums_old)
    taps = blocks._dgrad_taps(3, 3, 1)
    wpk, kp, kmode = ops._pack(wx, 1, taps, 4, 4)
    dx_new = ops.new_nhwc(n, c, h, w, dev)
    d = blocks._spade_x2map_dgrad_desc(dseg, wpk.data_ptr(), kp, kmode, taps, dx_new)
    assert call('ssg_spade_dgrad_modulate_ok', C.byref(d)) == 1
    # thin32_cin from 65536 pixels and 32 columns on, thin4_cin below
    assert call('ssg_conv2d_kernel_id', C.byref(d)) == (15 if p >= 65536 and w >= 32 else 12)
    call('ssg_spade_dgrad_modulate_f32', C.byref(d), ptr(dout), ops._ld(dout), ptr(gb), ops._ld(gb), sp())
    torch.cuda.synchronize()
    diff = (dx_new.double() - dx_old.double()).abs()
    print('dx: max |lean - old| %.3e, elements that differ %d of %d' % (diff.max().item(), int((diff > 0).sum().item()), diff.numel()))
    assert torch.equal(dx_new, dx_old)


def test_router_keeps_the_old_sequence_where_a_query_declines(pkg, monkeypatch):
    """No GPU: _spade_bwd_route on CPU tensors with the library's answers scripted."""
    blocks, ops = pkg.blocks, pkg.ops
    n, c, h, w, nh = 1, 64, 8, 8, 4
    x, gb, dout = (ops.new_nhwc(n, c, h, w, 'cpu', zero=True) for _ in range(3))
    seg = ops.new_nhwc(n, 3, h, w, 'cpu', zero=True); a = ops.new_nhwc(n, nh, h, w, 'cpu', zero=True)
    wx = torch.zeros(3, c, 3, 3); wgb = torch.zeros(2 * c, nh, 3, 3)
    asked = []

    def scripted(ok, wgrad_ids, conv_ids):
        wg, cv = list(wgrad_ids), list(conv_ids)

        def fake(name, *args):
            asked.append(name)
            if name == 'ssg_spade_dgrad_modulate_ok':
                return ok
            if name == 'ssg_conv2d_wgrad_kernel_id':
                return wg.pop(0)
            if name == 'ssg_conv2d_kernel_id':
                return cv.pop(0)
            if name == 'ssg_conv2d_split_bn':
                return 0
            raise AssertionError('the router may only query, it called %s' % name)
        return fake

    def route(ok, wgrad_ids, conv_ids, lean=2):
        del asked[:]
        monkeypatch.setattr(blocks, 'SPADE_BWD_LEAN', lean)
        monkeypatch.setattr(blocks, 'call', scripted(ok, wgrad_ids, conv_ids))
        return blocks._spade_bwd_route(x, seg, a, gb, dout, wx, wgb, 1)
    assert route(0, [50, 50, 50], [13, 13]) is False and asked == ['ssg_spade_dgrad_modulate_ok']  # _ok declines: old sequence
    assert route(1, [50, 50, 50], [13, 13]) is True
    assert route(1, [50, 50, 50], [2, 13]) is False              # the two-pointer launch would leave the one-pointer kernel
    assert route(1, [50, 51, 50], [13, 13]) is False             # the gamma half of the weight gradient would change kernel
    assert route(1, [50, 50, 21], [13, 13]) is False             # the beta half
    assert route(1, [50, 50, 50], [13, 13], lean=0) is False and asked == []                       # SSG_SPADE_BWD_LEAN=0
    # the default: 4096 elements are far below SPADE_BWD_LEAN_MIN, nothing is asked; with the bound lowered the queries decide
    assert route(1, [50, 50, 50], [13, 13], lean=1) is False and asked == []
    monkeypatch.setattr(blocks, 'SPADE_BWD_LEAN_MIN', n * h * w * c)
    assert route(1, [50, 50, 50], [13, 13], lean=1) is True
