"""Block-level autograd Functions with hand-written backward passes.

The reference expresses BasicBlock (archs.py:205-241) and SPADE (normalization.py:67-122) as
chains of stock torch ops and lets autograd add the gradients of tensors that are consumed
twice (block input -> conv1 and shortcut; SPADE input -> x2map and the modulation).  Here a
whole block is ONE autograd node: the backward pass is an explicit kernel schedule in which
those gradient sums ride the dgrad kernel's residual epilogue, the ReLU masks are folded into
the batch-norm backward kernels, and `torch.cat` never materialises (two-pointer convs).
"""
import ctypes as C
import os

import torch

from . import ops
from ._lib import ACT_NONE, ACT_RELU, call, ptr, stream_ptr
from .ops import (_act_bwd, _bn_bwd_impl, _bn_fwd_impl, _channel_sum, _conv_dgrad_impl, _conv_fwd_impl, _conv_wgrad_impl,
                  _ld, new_nhwc, to_nhwc)


# ----------------------------------------------------------------------------- ops.train_precision('bf16x1')
# `x1m` is the mode a node's FORWARD read (and its stride is 1): the node then passes precision='bf16x1' to its two 3x3 convs in
# all three directions.  Each launch runs on the one-term bf16 kernel only where its own predicate holds
# (ssg_conv2d_bf16x1_ok / ssg_conv2d_wgrad_bf16x1_ok: 64-channel multiples, >= 17 pixels wide); a refused launch runs on the
# fp32-class kernel it runs on today.  The 1x1 shortcut always passes 'fp32'.  train_precision('bf16x2') is handled alike: `x1m` is
# then 'bf16x2' and the launches ask the two-term kernels (ssg_conv2d_bf16x2_ok / ssg_conv2d_wgrad_bf16x2_ok, the same shapes).
def _x_mode(stride):
    """'bf16x1' / 'bf16x2' where train_precision names one and the block's stride is 1, else False."""
    mode = ops.train_precision_mode()
    return mode if mode != 'fp32' and stride == 1 else False


class _BasicBlockFn(torch.autograd.Function):
    """relu(bn1(conv3x3(x))) -> bn2(conv3x3(.)) -> (+ conv1x1(x) | + x) -> relu, x = cat(x1, x2)."""

    @staticmethod
    def forward(ctx, x1, x2, w1, g1, b1, rm1, rv1, w2, g2, b2, rm2, rv2, wsc, eps1, mom1, eps2, mom2, stride, var_mode, group):
        x1 = to_nhwc(x1)
        x2 = to_nhwc(x2) if x2 is not None else None
        ctx.x1m = x1m = _x_mode(stride)
        p3 = x1m or 'fp32'
        # batch-norm statistics ride the producing conv's epilogue where its kernel has one (part = None otherwise: the bf16x1
        # launcher has none, so behind a routed conv the batch norm runs its own statistics pass)
        c1, part1 = _conv_fwd_impl(x1, x2, w1, None, stride, 1, ACT_NONE, 0.0, want_bn=True, precision=p3)
        # relu(bn1(c1)) is applied on conv2's INPUT where its kernel can (the split-operand k32 tiles): y1 is never written, the
        # backward's weight gradient reads c1 through the same transform and the ReLU mask is recomputed from c1 as before.
        # Off under bf16x1, also for a block whose first conv was refused and so has a part1.
        y1 = None
        c2 = None
        if ops.BN_FUSE_INPUT and part1 is not None and not x1m:
            _, st1, cnt1 = _bn_fwd_impl(c1, g1, b1, rm1, rv1, None, eps1, mom1, ACT_RELU, 0.0, var_mode, group, part=part1, apply=False)
            r = _conv_fwd_impl(c1, None, w2, None, 1, 1, ACT_NONE, 0.0, want_bn=True, in_affine=(st1[2], st1[3], ACT_RELU, 0.0))
            if r is not None:
                c2, part2 = r
            else:
                with ops._hbm('bn_fwd', 8.0 * c1.numel()):
                    y1 = ops._bn_apply(c1, st1, None, ACT_RELU, 0.0)
        else:
            y1, st1, cnt1 = _bn_fwd_impl(c1, g1, b1, rm1, rv1, None, eps1, mom1, ACT_RELU, 0.0, var_mode, group, part=part1)
        if c2 is None:
            c2, part2 = _conv_fwd_impl(y1, None, w2, None, 1, 1, ACT_NONE, 0.0, want_bn=True, precision=p3)
        if wsc is not None:
            sc = _conv_fwd_impl(x1, x2, wsc, None, stride, 0, ACT_NONE, 0.0)
        else:
            if x2 is not None:
                raise ValueError('identity shortcut with a two-tensor input')
            sc = x1
        # the final ReLU's mask in C / 8 bytes per pixel where the kernels allow it (ops.BN_BWD_LEAN): `out` is then not kept
        out, st2, cnt2, mask = _bn_fwd_impl(c2, g2, b2, rm2, rv2, sc, eps2, mom2, ACT_RELU, 0.0, var_mode, group, part=part2, want_mask=True)
        ctx.save_for_backward(x1, x2, c1, y1, c2, out if mask is None else None, w1, g1, w2, g2, wsc, st1, st2, mask)   # y1 = None on the fused route
        ctx.cfg = (stride, group, cnt1, cnt2)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        x1, x2, c1, y1, c2, out, w1, g1, w2, g2, wsc, st1, st2, mask = ctx.saved_tensors
        stride, group, cnt1, cnt2 = ctx.cfg
        x1m = ctx.x1m                                    # the forward's train_precision mode, whatever is set now
        p3 = x1m or 'fp32'
        dout = to_nhwc(dout)
        n, ca, h, w = x1.shape
        cb = x2.shape[1] if x2 is not None else 0
        need_x1, need_x2 = ctx.needs_input_grad[0], (x2 is not None and ctx.needs_input_grad[1])
        # bn2 backward; dres = dout masked by the final ReLU = gradient of the shortcut branch
        dc2, g, dg2, db2 = _bn_bwd_impl(c2, out, dout, g2, st2, ACT_RELU, 0.0, group, cnt2, want_dres=True, mask=mask)
        if y1 is None:                                   # fused route: conv2 read relu(bn1(c1)) through its input transform
            dw2 = _conv_wgrad_impl(c1, None, dc2, w2.shape, 1, 1, in_affine=(st1[2], st1[3], ACT_RELU, 0.0))
            if dw2 is None:                              # no weight-gradient kernel with the transform for this shape: write y1 now
                with ops._hbm('bn_fwd', 8.0 * c1.numel()):
                    y1w = ops._bn_apply(c1, st1, None, ACT_RELU, 0.0)
                dw2 = _conv_wgrad_impl(y1w, None, dc2, w2.shape, 1, 1)
                del y1w
        else:
            dw2 = _conv_wgrad_impl(y1, None, dc2, w2.shape, 1, 1, precision=p3)
        # bn1's backward sums ride the epilogue of the input gradient that produces d(relu(bn1(c1))) where its kernel has one
        # (ssg_conv_desc.bwd_x: the k32 tiles): the reduce pass over (dy1, c1) goes, the apply pass reads the already masked gradient.
        # Off under bf16x1.
        r = _conv_dgrad_impl(dc2, w2, 1, 1, c1.shape[2], c1.shape[3], 0, c1.shape[1], bwd_stats=(c1, st1, ACT_RELU, 0.0)) \
            if ops.BN_BWD_EPILOGUE and not x1m else None
        if r is not None:
            dc1, dg1, db1 = ops._bn_bwd_from_partials(c1, r[0], r[1], g1, st1, group, cnt1)
        else:
            dy1 = _conv_dgrad_impl(dc2, w2, 1, 1, c1.shape[2], c1.shape[3], 0, c1.shape[1], precision=p3)
            dc1, _, dg1, db1 = _bn_bwd_impl(c1, y1, dy1, g1, st1, ACT_RELU, 0.0, group, cnt1, want_dres=False, had_res=False)
        dw1 = _conv_wgrad_impl(x1, x2, dc1, w1.shape, stride, 1, precision=p3)
        dwsc = _conv_wgrad_impl(x1, x2, g, wsc.shape, stride, 0) if wsc is not None else None
        dx1 = dx2 = None
        if stride != 1 and (need_x1 or need_x2):
            raise NotImplementedError('strided BasicBlock input gradient')
        if need_x1:
            part = _conv_dgrad_impl(g, wsc, 1, 0, h, w, 0, ca) if wsc is not None else g
            dx1 = _conv_dgrad_impl(dc1, w1, 1, 1, h, w, 0, ca, res=part, precision=p3)
        if need_x2:
            part = _conv_dgrad_impl(g, wsc, 1, 0, h, w, ca, ca + cb)
            dx2 = _conv_dgrad_impl(dc1, w1, 1, 1, h, w, ca, ca + cb, res=part, precision=p3)
        return (dx1, dx2, dw1, dg1, db1, None, None, dw2, dg2, db2, None, None, dwsc,
                None, None, None, None, None, None, None)


def _block_weights(op, x, conv1, conv2, shortcut_conv):
    """ops.param over the three conv weights of a BasicBlock (read only through ops._pack: they stay the Parameters themselves)."""
    return (ops.param(op, 'conv1.weight', conv1.weight, x, packed=True), ops.param(op, 'conv2.weight', conv2.weight, x, packed=True),
            ops.param(op, 'shortcut.weight', shortcut_conv.weight, x, packed=True) if shortcut_conv is not None else None)


def check_block_params(op, x, conv1, bn1, conv2, bn2, shortcut_conv):
    """The parameter contract (ops.param) over everything a BasicBlock holds, for the routes of archs.BasicBlock that fold or
    compose with torch ops before an entry point of this package sees the operands.  Checks only: returns nothing."""
    _block_weights(op, x, conv1, conv2, shortcut_conv)
    for name, bn in (('bn1', bn1), ('bn2', bn2)):
        ops.bn_params(op, bn, x, stats=bn.track_running_stats, name=name)


def basic_block(x1, x2, conv1, bn1, conv2, bn2, shortcut_conv, group=None):
    """Fused training-mode BasicBlock over nn.Conv2d / nn.BatchNorm2d parameter holders."""
    w1, w2, wsc = _block_weights('basic_block', x1, conv1, conv2, shortcut_conv)
    g1, b1, rm1, rv1 = ops.bn_params('basic_block', bn1, x1, stats=bn1.track_running_stats, name='bn1')
    g2, b2, rm2, rv2 = ops.bn_params('basic_block', bn2, x1, stats=bn2.track_running_stats, name='bn2')
    for bn in (bn1, bn2):
        # the reference's synchronised branch never touches num_batches_tracked (batchnorm.py:57-80); its stock branch does
        if bn.track_running_stats and bn.num_batches_tracked is not None and not ops._synced(group):
            bn.num_batches_tracked.add_(1)
    var_mode = getattr(bn1, '_ssg_var_mode', 1 if group is not None else 0)
    return _BasicBlockFn.apply(x1, x2, w1, g1, b1, rm1, rv1, w2, g2, b2, rm2, rv2, wsc,
                               float(bn1.eps), float(bn1.momentum), float(bn2.eps), float(bn2.momentum),
                               int(conv1.stride[0]), var_mode, group)


def _fold_bwd(dwf, w, s, mean, invstd, sums_g, need_w, need_gb):
    """(dw, dgamma, dbeta) through the fold Wf = W*s, bf = beta - mean*s (ssg_bn_fold_bwd_f32); only what is asked for."""
    o = w.shape[0]
    dw = torch.empty_like(dwf) if need_w else None
    dgb = torch.empty((2, o), dtype=torch.float32, device=w.device) if need_gb else None
    wc = w.detach().contiguous()
    call('ssg_bn_fold_bwd_f32', ptr(dwf), ptr(wc), o, wc.numel() // o, ptr(s), ptr(mean), ptr(invstd), ptr(sums_g), ptr(dw),
         ptr(dgb[0]) if need_gb else None, ptr(dgb[1]) if need_gb else None, stream_ptr())
    return dw, (dgb[0] if need_gb else None), (dgb[1] if need_gb else None)


class _FrozenBasicBlockFn(torch.autograd.Function):
    """BasicBlock whose two batch norms use their running statistics (eval mode / batchnorm.freeze_batch_norm), with autograd:
    relu(conv3x3(x, Wf1) + bf1) -> relu(conv3x3(., Wf2) + bf2 + (conv1x1(x) | x)), Wf = W * gamma*invstd, bf = beta - mean*gamma*invstd.
    The forward is the three launches of the eval branch of archs.BasicBlock (same kernels, same bits); no batch-norm pass runs in
    either direction.  Saved: x1, x2, y1, out -- the two conv outputs of the train node (c1, c2) and its statistics never exist.
    k1 / k2 = (s, mean, invstd) of bn1 / bn2."""

    @staticmethod
    def forward(ctx, x1, x2, w1, g1, b1, w2, g2, b2, wsc, wf1, bf1, wf2, bf2, k1, k2, stride, record):
        x1 = to_nhwc(x1)
        x2 = to_nhwc(x2) if x2 is not None else None
        # train_precision('bf16x1'): the folded convs with their bias / ReLU / residual epilogues on the bf16x1 kernel, as the eval
        # path under infer_precision; only a forward that records a graph reads the mode
        x1m = record and any(ctx.needs_input_grad) and _x_mode(stride)
        p3 = x1m or 'fp32'
        y1 = _conv_fwd_impl(x1, x2, wf1, bf1, stride, 1, ACT_RELU, 0.0, precision=p3)
        if wsc is not None:
            r = _conv_fwd_impl(x1, x2, wsc, None, stride, 0, ACT_NONE, 0.0)
        else:
            if x2 is not None:
                raise ValueError('identity shortcut with a two-tensor input')
            r = x1
        out = _conv_fwd_impl(y1, None, wf2, bf2, 1, 1, ACT_RELU, 0.0, res=r, precision=p3)
        if record and any(ctx.needs_input_grad):          # `record`: the caller's grad mode (it is always off inside forward)
            ctx.save_for_backward(x1, x2, y1, out, w1, w2, wsc, wf1, wf2, *k1, *k2)
            ctx.stride = stride
            ctx.x1m = x1m
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        x1, x2, y1, out, w1, w2, wsc, wf1, wf2, s1, m1, is1, s2, m2, is2 = ctx.saved_tensors
        stride = ctx.stride
        p3 = ctx.x1m or 'fp32'                           # the forward's train_precision mode, whatever is set now
        dout = to_nhwc(dout)
        n, ca, h, w = x1.shape
        cb = x2.shape[1] if x2 is not None else 0
        need = ctx.needs_input_grad
        need_x1, need_x2 = need[0], (x2 is not None and need[1])
        need_w1, need_gb1, need_w2, need_gb2 = need[2], (need[3] or need[4]), need[5], (need[6] or need[7])
        need_wsc = wsc is not None and need[8]
        if stride != 1 and (need_x1 or need_x2):
            raise NotImplementedError('strided BasicBlock input gradient')
        # final ReLU: g2 = dout masked by out > 0 and its column sums (= d bf2) in one pass; g2 is also the shortcut branch's gradient
        g2, _, sums2 = ops._frozen_bwd(None, out, dout, None, None, None, None, ACT_RELU, 0.0)
        dw2 = dg2 = db2 = None
        if need_w2 or need[6]:
            dwf2 = _conv_wgrad_impl(y1, None, g2, w2.shape, 1, 1, precision=p3)
            dw2, dg2, db2 = _fold_bwd(dwf2, w2, s2, m2, is2, sums2, need_w2, need_gb2)
        elif need_gb2:
            db2 = sums2[:w2.shape[0]].float()
        dwsc = _conv_wgrad_impl(x1, x2, g2, wsc.shape, stride, 0) if need_wsc else None
        dw1 = dg1 = db1 = dx1 = dx2 = None
        if need_w1 or need_gb1 or need_x1 or need_x2:
            dy1 = _conv_dgrad_impl(g2, wf2, 1, 1, y1.shape[2], y1.shape[3], 0, y1.shape[1], precision=p3)
            g1, _, sums1 = ops._frozen_bwd(None, y1, dy1, None, None, None, None, ACT_RELU, 0.0)
            del dy1
            if need_w1 or need[3]:
                dwf1 = _conv_wgrad_impl(x1, x2, g1, w1.shape, stride, 1, precision=p3)
                dw1, dg1, db1 = _fold_bwd(dwf1, w1, s1, m1, is1, sums1, need_w1, need_gb1)
            elif need_gb1:
                db1 = sums1[:w1.shape[0]].float()
            # the shortcut's gradient rides the residual epilogue of conv1's input gradient, as in _BasicBlockFn
            if need_x1:
                part = _conv_dgrad_impl(g2, wsc, 1, 0, h, w, 0, ca) if wsc is not None else g2
                dx1 = _conv_dgrad_impl(g1, wf1, 1, 1, h, w, 0, ca, res=part, precision=p3)
            if need_x2:
                part = _conv_dgrad_impl(g2, wsc, 1, 0, h, w, ca, ca + cb)
                dx2 = _conv_dgrad_impl(g1, wf1, 1, 1, h, w, ca, ca + cb, res=part, precision=p3)
        return (dx1, dx2, dw1, dg1 if need[3] else None, db1 if need[4] else None, dw2, dg2 if need[6] else None,
                db2 if need[7] else None, dwsc, None, None, None, None, None, None, None, None)


def frozen_basic_block(x1, x2, conv1, bn1, conv2, bn2, shortcut_conv, folded, consts):
    """BasicBlock over frozen batch norms as one autograd node.  `folded` = (wf1, bf1, wf2, bf2) and `consts` =
    ((s1, mean1, invstd1), (s2, mean2, invstd2)) come from archs.BasicBlock's caches; nothing here writes a running statistic."""
    wf1, bf1, wf2, bf2 = folded
    w1, w2, wsc = _block_weights('frozen_basic_block', x1, conv1, conv2, shortcut_conv)
    g1, b1, _, _ = ops.bn_params('frozen_basic_block', bn1, x1, name='bn1')
    g2, b2, _, _ = ops.bn_params('frozen_basic_block', bn2, x1, name='bn2')
    return _FrozenBasicBlockFn.apply(x1, x2, w1, g1, b1, w2, g2, b2, wsc, wf1, bf1, wf2, bf2,
                                     consts[0], consts[1], int(conv1.stride[0]), torch.is_grad_enabled())


def _spade_cat(wg, bg, wb, bb):
    """gamma and beta convs as ONE conv nhidden -> 2C: weights / biases concatenated along the output channels.  Cached on
    the gamma weight for one (storage, version, optimizer epoch) of the four tensors, so an eval loop concatenates once."""
    stamp = ops._stamp((wg, bg, wb, bb))
    hit = wg.__dict__.get('_ssg_gb_cat')
    if hit is not None and hit[0] == stamp:
        return hit[1], hit[2]
    with torch.no_grad():
        w = torch.cat([wg.detach(), wb.detach()], 0).contiguous()
        b = torch.cat([bg.detach(), bb.detach()], 0).contiguous()
    ops._attach(wg, '_ssg_gb_cat', (stamp, w, b))
    return w, b


def _spade_fused_fwd(x, a, wgb, bgb, pad, out):
    """gamma|beta conv + modulation in one kernel (ssg_spade_conv_modulate_f32) where the shape allows it (4- or 8-channel `a`,
    3x3, >= 65536 pixels: the 512^2 and 256^2 levels at batch 16).  Writes `out`, returns gamma (needed by the backward) or None."""
    o, i, kh, kw = wgb.shape
    n, c, h, w = x.shape
    cin = ops.pad4(a.shape[1])
    if kh != 3 or kw != 3 or pad != 1 or cin not in (4, 8) or o != 2 * c or c % 4:
        return None
    taps = ops._taps_fwd(kh, kw, pad)
    wpk, kp, kmode = ops._pack(wgb, 0, taps, cin, cin)
    d = ops._conv_desc(ops._at(a), cin, None, 0, (n, h, w), wpk.data_ptr(), kp, kmode, bgb, None, ops._at(out), o,
                       (h, w, h, w), 1, 1, (0, 0), taps, ACT_NONE, 0.0)
    if not call('ssg_spade_conv_modulate_ok', C.byref(d)):
        return None
    gamma = new_nhwc(n, c, h, w, x.device)
    with ops._Timed('thin32_cin_kernel<spade>' if ops.PROFILE is not None else None, 2.0 * n * h * w * o * a.shape[1] * 9):
        call('ssg_spade_conv_modulate_f32', C.byref(d), ptr(x), _ld(x), ptr(gamma), _ld(gamma), stream_ptr())
    return gamma


# SSG_SPADE_BWD_LEAN (like SSG_K32): 0 = every SPADE layer runs the backward that writes dx = dout*(1+gamma) and the
# d(gamma)|d(beta) tensor (12 passes over an [N,C,H,W] tensor per layer); 1 = the lean one (10: DESIGN.md 3.24) where its kernels
# allow it and the tensor has at least SPADE_BWD_LEAN_MIN elements; 2 = wherever its kernels allow it (tests).
# Below 2^20 elements the three passes the lean sequence saves are under 12 MB, under 3 us at the 5 TB/s these passes reach:
# less than the launch of the second weight-gradient kernel and its reduce stage that the lean sequence adds.
SPADE_BWD_LEAN = {'0': 0, '2': 2}.get(os.environ.get('SSG_SPADE_BWD_LEAN', '1'), 1)
SPADE_BWD_LEAN_MIN = 1 << 20
# The batch-norm backward has the same kind of switch, SSG_BN_BWD_LEAN, and its threshold ops.BN_BWD_LEAN_MIN: they live in ops.py,
# beside the nodes that read them (ops._BatchNormAct, ops._ConvBnAct, ops._Conv2d); _BasicBlockFn above asks through _bn_fwd_impl.


def _dgrad_taps(kh, kw, pad):
    pt, _, pl, _ = ops._pad4(pad)
    return [(ky, kx, pt - ky, pl - kx) for ky in range(kh) for kx in range(kw)]


def _pack_shape(ntaps, cred_pad):
    """(Kp, kmode) ops._pack gives a weight packed over `cred_pad` reduced channels (without packing anything)."""
    kmode = 0 if cred_pad % 16 == 0 else 1
    return (ntaps * cred_pad if kmode == 0 else (ntaps * cred_pad + 15) // 16 * 16), kmode


def _conv_route_id(d, kmode):
    """ssg_conv2d_kernel_id of descriptor `d` as ops._conv_launch would launch it (the split pack's stand-in included)."""
    pack = call('ssg_conv2d_split_bn', C.byref(d)) if ops.MFMA_SPLIT and kmode == 0 else 0
    d.w_split = 1 if pack else None
    return call('ssg_conv2d_kernel_id', C.byref(d))


def _spade_x2map_dgrad_desc(dseg, wpk_ptr, kp, kmode, taps, dx):
    """The x2map input gradient (padded label_nc -> C channels) as ssg_conv2d_f32 launches it, without a residual."""
    n, c, h, w = dx.shape
    return ops._conv_desc(ops._at(dseg), ops.pad4(dseg.shape[1]), None, 0, (n, h, w), wpk_ptr, kp, kmode, None, None, ops._at(dx), c,
                          (h, w, h, w), 1, 1, (0, 0), taps, ACT_NONE, 0.0)


def _spade_bwd_route(x, seg, a, gb, dout, wx, wgb, pad):
    """Which backward one SPADE layer runs -- the one place that decides it: True, the lean sequence, or
    False, the old one (the modulate pass writes dx = dout*(1+gamma) and the d(gamma)|d(beta) tensor).  The lean sequence needs
      * a tensor large enough to gain from it (SPADE_BWD_LEAN_MIN; not under SPADE_BWD_LEAN = 2),
      * the x2map input gradient on a kernel with the modulated-residual epilogue (ssg_spade_dgrad_modulate_ok),
      * each C-channel half of the gamma|beta weight gradient on the kernel the 2C-channel launch runs on
        (ssg_conv2d_wgrad_kernel_id),
      * the input gradient of the gamma|beta conv, reading d(gamma) and dout through the descriptor's two input pointers, on
        the kernel the one-pointer launch over d(gamma)|d(beta) runs on (ssg_conv2d_kernel_id: same kernel, same order of
        the reduction, same bits), and
      * dout / gamma the epilogue's buffer descriptors can address (under 2^30 elements; nhwc_ld has checked the rest).
    Only host-side queries: nothing is allocated, packed or launched here (the stand-in pointers are never read)."""
    if not SPADE_BWD_LEAN:
        return False
    n, c, h, w = x.shape
    nh = a.shape[1]
    if SPADE_BWD_LEAN == 1 and n * h * w * c < SPADE_BWD_LEAN_MIN:
        return False
    if c % 4 or n * h * w * max(_ld(dout), _ld(gb), _ld(x)) >= 1 << 30:
        return False
    kh, kw = wx.shape[2], wx.shape[3]
    taps = _dgrad_taps(kh, kw, pad)
    kp, kmode = _pack_shape(len(taps), ops.pad4(seg.shape[1]))
    if not call('ssg_spade_dgrad_modulate_ok', C.byref(_spade_x2map_dgrad_desc(seg, seg.data_ptr(), kp, kmode, taps, x))):
        return False
    gkh, gkw = wgb.shape[2], wgb.shape[3]

    def wgrad_id(cout, ldd):
        d = ops._wgrad_desc(a, ops.pad4(nh), None, 0, dout, (cout, nh, gkh, gkw), 1, ops._taps_fwd(gkh, gkw, pad))
        d.ldd = ldd
        d.dw_oihw = dout.data_ptr(); d.flags = 1 if ops.MFMA_SPLIT else 0
        return call('ssg_conv2d_wgrad_kernel_id', C.byref(d))

    whole = wgrad_id(2 * c, 2 * c)
    if wgrad_id(c, c) != whole or wgrad_id(c, _ld(dout)) != whole:
        return False
    gtaps = _dgrad_taps(gkh, gkw, pad)
    kp, kmode = _pack_shape(len(gtaps), 2 * c)

    def dgrad_id(in1, c1, in2, c2):
        return _conv_route_id(ops._conv_desc(in1, c1, in2, c2, (n, h, w), x.data_ptr(), kp, kmode, None, None, ops._at(a), nh,
                                             (h, w, h, w), 1, 1, (0, 0), gtaps, ACT_NONE, 0.0), kmode)

    p = x.data_ptr()
    return dgrad_id((p, c), c, (dout.data_ptr(), _ld(dout)), c) == dgrad_id((p, 2 * c), 2 * c, None, 0)


class _SpadeFn(torch.autograd.Function):
    """Self-conditioned SPADE: out = x*(1+gamma(a)) + beta(a), a = relu(shared(x2map(x))).
    gamma and beta come from one conv nhidden -> 2C (concatenated weights) writing gamma|beta pixel rows.  Backward
    (_spade_bwd_route says where): d(beta) = dout is not copied and dx = dout*(1+gamma) is not stored -- the modulate pass writes d(gamma) and
    the bias sums only, the consumers of d(gamma)|d(beta) take their two halves from d(gamma) and dout, and the product joins dx
    in the epilogue of the x2map input gradient.  Where a layer's kernels do not allow that, the old sequence: the input
    gradient of the gamma|beta conv is one launch with K = 9*2C and its weight gradient one launch whose halves are d(gamma), d(beta)."""

    @staticmethod
    def forward(ctx, x, wx, bx, ws, bs, wg, bg, wb, bb, pad):
        x = to_nhwc(x)
        n, c, h, w = x.shape
        seg = _conv_fwd_impl(x, None, wx, bx, 1, pad, ACT_NONE, 0.0)
        a = _conv_fwd_impl(seg, None, ws, bs, 1, pad, ACT_RELU, 0.0)
        wgb, bgb = _spade_cat(wg, bg, wb, bb)
        out = new_nhwc(n, c, h, w, x.device)
        gb = _spade_fused_fwd(x, a, wgb, bgb, pad, out)           # gamma only ([n, c, h, w]) when the fused kernel took it
        if gb is None:
            gb = _conv_fwd_impl(a, None, wgb, bgb, 1, pad, ACT_NONE, 0.0)
            with ops._hbm('spade_modulate_fwd', 16.0 * n * h * w * c):           # x, gamma, beta in; out (3 reads + 1 write)
                call('ssg_spade_modulate_fwd_f32', ptr(x), _ld(x), ptr(gb), _ld(gb), n * h * w, c, ptr(out), _ld(out), stream_ptr())
        ctx.save_for_backward(x, seg, a, gb, wx, ws, wgb)
        ctx.pad = pad
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        x, seg, a, gb, wx, ws, wgb = ctx.saved_tensors
        pad = ctx.pad
        dout = to_nhwc(dout)
        n, c, h, w = x.shape
        nh = a.shape[1]
        lean = _spade_bwd_route(x, seg, a, gb, dout, wx, wgb, pad)
        # modulate backward and the gamma / beta bias gradients (column sums of d(gamma), d(beta)) in one pass over the data
        scratch = ops._ws(call('ssg_bn_workspace_bytes', n * h * w, c), x.device)
        sums = torch.empty(2 * c, dtype=torch.float64, device=x.device)
        if lean:
            # the 10-pass sequence: neither dx = dout*(1+gamma) nor d(gamma)|d(beta) exists.  x, dout in; d(gamma) out
            dgamma = new_nhwc(n, c, h, w, x.device)
            with ops._hbm('spade_modulate_bwd', 4.0 * n * h * w * c * (2 + 1)):
                call('ssg_spade_modulate_dgamma_sums_f32', ptr(x), _ld(x), ptr(dout), _ld(dout), n * h * w, c, ptr(dgamma), _ld(dgamma),
                     ptr(sums), ptr(scratch), stream_ptr())
            half = (c,) + tuple(wgb.shape[1:])               # the shape of the gamma conv's weight, and of the beta conv's
            dwg = _conv_wgrad_impl(a, None, dgamma, half, 1, pad)
            dwb = _conv_wgrad_impl(a, None, dout, half, 1, pad)
            # the input gradient over the concatenated pack of wgb: channels [0, C) from d(gamma), [C, 2C) from dout
            taps = _dgrad_taps(wgb.shape[2], wgb.shape[3], pad)
            wpk, kp, kmode = ops._pack(wgb, 1, taps, 2 * c, 2 * c)
            da = new_nhwc(n, nh, h, w, x.device)
            ops._conv_launch(dgamma, dout, wpk, kp, kmode, 0, nh, None, None, ACT_NONE, 0.0, taps, n, h, w, h, w, h, w, 1, 1, 0, 0, da)
            del dgamma
        else:
            dxm = new_nhwc(n, c, h, w, x.device)
            dgb = new_nhwc(n, 2 * c, h, w, x.device)
            # x, gamma (|beta where the conv wrote both), dout in; dx, d(gamma), d(beta) out
            with ops._hbm('spade_modulate_bwd', 4.0 * n * h * w * c * (3 + 3)):
                call('ssg_spade_modulate_bwd_sums_f32', ptr(x), _ld(x), ptr(gb), _ld(gb), ptr(dout), _ld(dout), n * h * w, c,
                     ptr(dxm), _ld(dxm), ptr(dgb), _ld(dgb), ptr(sums), ptr(scratch), stream_ptr())
            dwgb = _conv_wgrad_impl(a, None, dgb, wgb.shape, 1, pad)
            dwg, dwb = dwgb[:c], dwgb[c:]
            da = _conv_dgrad_impl(dgb, wgb, 1, pad, h, w, 0, nh)
            del dgb
        dbias_gb = sums.float()
        da = _act_bwd(a, da, ACT_RELU, 0.0)
        dws = _conv_wgrad_impl(seg, None, da, ws.shape, 1, pad)
        dbs = _channel_sum(da, nh)
        dseg = _conv_dgrad_impl(da, ws, 1, pad, h, w, 0, seg.shape[1])
        dwx = _conv_wgrad_impl(x, None, dseg, wx.shape, 1, pad)
        dbx = _channel_sum(dseg, seg.shape[1])
        dx = None
        if ctx.needs_input_grad[0] and lean:
            # dx = dgrad(dseg, wx) + dout*(1+gamma): the product is formed in the launch's epilogue (only the gamma half of gb is read)
            kh, kw = wx.shape[2], wx.shape[3]
            taps = _dgrad_taps(kh, kw, pad)
            cred = ops.pad4(wx.shape[0])
            wpk, kp, kmode = ops._pack(wx, 1, taps, cred, cred)
            dx = new_nhwc(n, c, h, w, x.device)
            d = _spade_x2map_dgrad_desc(dseg, wpk.data_ptr(), kp, kmode, taps, dx)
            label = ops._CONV_LABELS.get(call('ssg_conv2d_kernel_id', C.byref(d)), '?') if ops.PROFILE is not None else None
            with ops._Timed(label, 2.0 * n * h * w * c * wx.shape[0] * kh * kw):
                call('ssg_spade_dgrad_modulate_f32', C.byref(d), ptr(dout), _ld(dout), ptr(gb), _ld(gb), stream_ptr())
        elif ctx.needs_input_grad[0]:
            dx = _conv_dgrad_impl(dseg, wx, 1, pad, h, w, 0, c, res=dxm)
        return dx, dwx, dbx, dws, dbs, dwg, dbias_gb[:c], dwb, dbias_gb[c:], None


def spade_self(x, x2map, shared, gamma, beta):
    """Fused SPADE(x, x) over the four nn.Conv2d parameter holders."""
    args = []
    for name, conv in (('x2map', x2map), ('mlp_shared', shared), ('mlp_gamma', gamma), ('mlp_beta', beta)):
        args += [ops.param('spade_self', name + '.weight', conv.weight, x, packed=True), ops.param('spade_self', name + '.bias', conv.bias, x)]
    return _SpadeFn.apply(x, *args, int(x2map.padding[0]))
