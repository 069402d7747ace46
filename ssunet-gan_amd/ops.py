"""Autograd ops over the gfx950 C-ABI (include/ssunet_hip.h).  Every op here launches a
hand-written HIP kernel; none falls back to a stock torch compute op, and all of them raise
if the tensors are not on a HIP device or the shared library is not built.

Tensor convention ("NHWC-with-stride"): an activation is a torch tensor of logical shape
[N, C, H, W] whose memory is [N, H, W, ld] with ld = C rounded up to 4 (pad channels are
zero).  For C % 4 == 0 this is exactly torch.channels_last, so tensors stay ordinary torch
tensors at the nn.Module boundary while the kernels see coalesced channel rows.
"""
import ctypes as C
import math

import torch
import torch.distributed as dist

from . import _lib
from ._lib import ACT_LRELU, ACT_NONE, ACT_RELU, ACT_SWISH, ConvDesc, WgradDesc, call, ptr, stream_ptr

__all__ = ['conv2d', 'batch_norm_act', 'max_pool2x2', 'max_pool2x2_skip', 'max_unpool2x2', 'upsample2x_bilinear', 'upsample2x_nearest',
           'spade_modulate', 'adaptive_avgpool_flat', 'linear', 'seg_loss', 'bce_with_logits_const', 'nan_to_zero_',
           'to_nhwc', 'new_nhwc', 'bump_weight_epoch', 'dwconv2d', 'swish', 'sigmoid', 'gaussian', 'mul', 'global_avgpool',
           'channel_scale', 'spectral_norm_weight', 'conv2d_sn']


def pad4(c):
    return (c + 3) // 4 * 4


# ----------------------------------------------------------------------------- layout helpers
def new_nhwc(n, c, h, w, device, ld=None, zero=False):
    """Fresh [n, c, h, w] tensor over an [n, h, w, ld] buffer.  Built with set_() on the buffer's
    storage so the result is a base tensor, not an autograd view (callers may modify it in place,
    e.g. train_seg_gan.py:190), while the storage still covers the trailing pad lanes."""
    ld = pad4(c) if ld is None else ld
    buf = (torch.zeros if zero else torch.empty)(n * h * w * ld, device=device, dtype=torch.float32)
    return torch.empty(0, device=device, dtype=torch.float32).set_(
        buf.untyped_storage(), 0, (n, c, h, w), (h * w * ld, 1, w * ld, ld))


def nhwc_ld(x):
    """Pixel stride ld if x is NHWC-with-stride (and usable by the kernels), else None."""
    if x.dim() != 4 or x.dtype != torch.float32:
        return None
    n, c, h, w = x.shape
    s = x.stride()
    if w > 1:
        ld = s[3]
    elif h > 1:
        ld = s[2]
    elif n > 1:
        ld = s[0]
    else:
        ld = pad4(c)
    if ld % 4 or ld < c or (c > 1 and s[1] != 1):
        return None
    if (w > 1 and s[3] != ld) or (h > 1 and s[2] != w * ld) or (n > 1 and s[0] != h * w * ld):
        return None
    if c % 4 and ld != pad4(c):          # padded tensors must be our own (zero pad lanes)
        return None
    if x.data_ptr() % 16:
        return None
    return ld


def to_nhwc(x):
    """Return x in NHWC-with-stride form (no copy if it already is)."""
    _lib.require_gpu(x)
    if nhwc_ld(x) is not None:
        return x
    if x.dtype != torch.float32:
        raise TypeError('ssunet-gan_amd ops are fp32; got %s' % x.dtype)
    src = x.detach()
    if not src.is_contiguous():
        src = src.contiguous()
    n, c, h, w = src.shape
    out = new_nhwc(n, c, h, w, x.device)
    call('ssg_nchw_to_nhwc_f32', ptr(src), n, c, h, w, ptr(out), pad4(c), stream_ptr())
    return out


class _ToNHWC(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return to_nhwc(x)

    @staticmethod
    def backward(ctx, g):
        return g


def as_nhwc(x):
    """Differentiable layout normalisation used at module boundaries."""
    if nhwc_ld(x) is not None:
        return x
    return _ToNHWC.apply(x) if x.requires_grad else to_nhwc(x)


def _ld(x):
    ld = nhwc_ld(x)
    if ld is None:
        raise _lib.HipLibraryError('internal: tensor is not NHWC-with-stride: shape %s stride %s' % (tuple(x.shape), x.stride()))
    return ld


# ----------------------------------------------------------------------------- parameter contract
def param(op, name, t, like=None, written=False, packed=False):
    """Check the non-activation operand `name` of public entry `op` (a weight, bias, batch-norm affine or running statistic, u / v)
    before anything is launched, and return what the kernels may read through data_ptr(): fp32, on the device of `like` (the
    activation; None: any HIP device), dense.  A dense fp32 operand -- every parameter of the training step -- comes back as
    itself.  A strided one comes back as a dense copy (`.contiguous()`, differentiable: its gradient reaches the original), except
      * written=True (running statistics, u / v: the kernels write them in place, a copy would swallow the update): ValueError;
      * packed=True (a weight read only through _pack / bf16._pack, which densify when they pack): the operand itself, so the
        packs stay stamped on the Parameter and no cache is ever keyed on a temporary.
    TypeError for another dtype, HipLibraryError for another device: a kernel would misread the one and fault on the other."""
    if t is None:
        return None
    if t.dtype != torch.float32:
        raise TypeError('%s: %s must be float32 (parameters and statistics are fp32 in every tensor family); got %s' % (op, name, t.dtype))
    if not t.is_cuda or (like is not None and t.device != like.device):
        raise _lib.HipLibraryError('%s: %s is on %s; it must be on %s (there is no CPU fallback and no peer access)' % (
            op, name, t.device, "the input's HIP device" if like is None or not like.is_cuda else like.device))
    if packed or t.is_contiguous():
        return t
    if written:
        raise ValueError('%s: %s is written in place and must be dense; got shape %s stride %s' % (op, name, tuple(t.shape), t.stride()))
    return t.contiguous()


def bn_params(op, bn, like, stats=True, name='bn'):
    """param() over the batch-norm module the caller calls `name`: (weight, bias, running_mean, running_var), the statistics
    None unless `stats`."""
    rm = bn.running_mean if stats else None
    rv = bn.running_var if stats else None
    return (param(op, name + '.weight', bn.weight, like), param(op, name + '.bias', bn.bias, like),
            param(op, name + '.running_mean', rm, like, written=True), param(op, name + '.running_var', rv, like, written=True))


def _dense(t):
    """`t` as the pack kernels read it: itself when dense, else a detached dense copy (made at pack time only, never cached)."""
    return t if t.is_contiguous() else t.detach().contiguous()


def _ws(nbytes, device):
    return torch.empty((max(int(nbytes), 16) + 15) // 16 * 2, dtype=torch.float64, device=device)


# ----------------------------------------------------------------------------- weight packing cache
_WEIGHT_EPOCH = [0]


def bump_weight_epoch():
    """Called by the fused optimizer (which writes parameters through raw pointers, invisible
    to tensor version counters) to invalidate packed-weight caches."""
    _WEIGHT_EPOCH[0] += 1


def _attach(t, name, value):
    try:
        setattr(t, name, value)
    except Exception:                            # exotic tensor subclasses: just do not cache
        pass
    return value


def _stamp(tensors, stats=False):
    """What every cache of tensors derived from parameters is valid for: the (storage address, autograd version) of each source,
    the optimizer epoch and, with `stats`, the running-statistics epoch (_STATS_EPOCH).  The one stamp of the package."""
    return tuple((t.data_ptr(), t._version) for t in tensors) + ((_WEIGHT_EPOCH[0], _STATS_EPOCH[0]) if stats else (_WEIGHT_EPOCH[0],))


def _stamped_cache(t, name):
    """The dict kept as attribute `name` ON tensor `t` (never keyed by address alone: a freed tensor's address can be reused by
    another weight), as (stamp, dict).  It is valid for one (storage address, autograd version, optimizer epoch) of `t`: a new
    stamp starts an empty dict."""
    stamp = _stamp((t,))
    cache = t.__dict__.get(name)
    if cache is None or cache[0] != stamp:
        cache = _attach(t, name, (stamp, {}))
    return cache[1]


def _pad4(pad):
    """int (symmetric) or (top, bottom, left, right) -> (pt, pb, pl, pr)."""
    if isinstance(pad, (tuple, list)):
        pt, pb, pl, pr = [int(v) for v in pad]
        return pt, pb, pl, pr
    return int(pad), int(pad), int(pad), int(pad)


def _taps_fwd(kh, kw, pad):
    pt, _, pl, _ = _pad4(pad)
    return [(ky, kx, ky - pt, kx - pl) for ky in range(kh) for kx in range(kw)]


def _pack(weight, transpose, taps, cred_pad, c1_for_mode, sigma=None):
    """Pack an OIHW weight for the given tap list; returns (tensor[R, Kp], Kp, kmode).  `sigma` (device scalar): pack
    weight / sigma instead (spectral norm; sigma changes every training forward, so this pack is not cached)."""
    o, i, kh, kw = weight.shape
    nt = len(taps)
    kmode = 0 if (cred_pad % 16 == 0 and c1_for_mode % 16 == 0) else 1
    kp = nt * cred_pad if kmode == 0 else (nt * cred_pad + 15) // 16 * 16
    rows = i if transpose else o
    if sigma is not None:
        out = torch.empty((rows, kp), device=weight.device, dtype=torch.float32)
        ky = (C.c_int * nt)(*[t[0] for t in taps]); kx = (C.c_int * nt)(*[t[1] for t in taps])
        wc = _dense(weight)
        call('ssg_pack_weights_scaled_f32', ptr(wc), o, i, kh, kw, int(transpose), nt, ky, kx, kmode, cred_pad, kp, ptr(sigma), ptr(out), stream_ptr())
        return out, kp, kmode
    cache = _stamped_cache(weight, '_ssg_pack')
    key = (transpose, tuple(taps), cred_pad, kmode)
    hit = cache.get(key)
    if hit is not None:
        return hit, kp, kmode
    out = torch.empty((rows, kp), device=weight.device, dtype=torch.float32)
    ky = (C.c_int * nt)(*[t[0] for t in taps])
    kx = (C.c_int * nt)(*[t[1] for t in taps])
    call('ssg_pack_weights_f32', ptr(_dense(weight)), o, i, kh, kw, int(transpose), nt, ky, kx, kmode, cred_pad, kp, ptr(out), stream_ptr())
    cache[key] = out
    return out, kp, kmode


def _fill_taps(desc, taps):
    desc.ntaps = len(taps)
    for t, (_, _, dy, dx) in enumerate(taps):
        desc.dy[t] = dy
        desc.dx[t] = dx


def _at(t):
    """(pointer, pixel stride) of an NHWC-with-stride tensor."""
    return t.data_ptr(), _ld(t)


def _conv_desc(in1, c1, in2, c2, nhw, w, kp, kmode, bias, res, out, cout, grid, in_s, out_s, out_o, taps, act, slope):
    """ssg_conv_desc with the fields every launch sets.  in1 / in2 / res / out: (pointer, pixel stride) pairs (in2, res: or None);
    c1 / c2, the pointers and `w` go in as given (padded counts and real pointers in _conv_launch, unpadded counts and stand-in
    pointers in _x1_desc).  grid = (GH, GW, OH, OW).  Everything else (bnpart, ws, w_split, parity_merge, in_*, bwd_*) keeps the
    structure's zero default for the caller that needs it."""
    d = ConvDesc()
    d.in1, d.ld1 = in1; d.C1 = c1
    if in2 is not None:
        d.in2, d.ld2 = in2; d.C2 = c2
    d.N, d.H, d.W = nhw
    d.w = w; d.Kp = kp; d.kmode = kmode
    d.bias = bias.data_ptr() if bias is not None else None
    if res is not None:
        d.res, d.ldr = res
    d.out, d.ldo = out; d.Cout = cout
    d.GH, d.GW, d.OH, d.OW = grid
    d.in_sy = d.in_sx = in_s
    d.out_sy = d.out_sx = out_s
    d.out_oy, d.out_ox = out_o
    _fill_taps(d, taps)
    d.act = act; d.slope = slope
    return d


def _wgrad_desc(x1, c1, x2, c2, dy, weight_shape, stride, taps):
    """ssg_wgrad_desc of dW[weight_shape] from cat(x1, x2) and dy; c1 / c2 go in as given (padded for the fp32-class kernels,
    unpadded for bf16x1).  flags, in_scale... and dw_oihw / ws are the caller's."""
    o, i, kh, kw = weight_shape
    d = WgradDesc()
    d.in1, d.ld1 = _at(x1); d.C1 = c1
    if x2 is not None:
        d.in2, d.ld2 = _at(x2); d.C2 = c2
    d.N, d.H, d.W = x1.shape[0], x1.shape[2], x1.shape[3]
    d.dout, d.ldd = _at(dy); d.Cout = o; d.GH, d.GW = dy.shape[2], dy.shape[3]
    d.in_sy = d.in_sx = stride
    _fill_taps(d, taps)
    for t, (ky, kx, _, _) in enumerate(taps):
        d.ky[t] = ky; d.kx[t] = kx
    d.KH, d.KW, d.Cin_real = kh, kw, i
    return d


# Optional per-launch timing (bench.py): a list that receives (kernel label, algorithmic FLOPs,
# start event, end event) for every MFMA conv launch, recorded on the launch stream.
PROFILE = None
PROFILE_SHAPES = False      # debug: append the launch geometry to the label
# bench.py's north-star sub-metrics (BASELINE.json: "MFMA roofline on the 3x3 encoder convs", "achieved HBM GB/s on the
# memory-bound upsample/BN stages"): while PROFILE is a list, PROFILE_HBM receives (stage, algorithmic bytes per SURVEY.md 8(d),
# start event, end event) for every launch group of the memory-bound stages, and every MFMA record carries the ROLE the model
# code set around the launch (archs.UNet_R_SS_v2 tags the forward 3x3 convs of its six encoder BasicBlocks 'encoder_3x3').
PROFILE_HBM = None
PROFILE_COMM = None         # (kind, bytes, start event, end event) per small collective on the compute stream (sync-BN statistics)
_ROLE = [None]


def _timed_all_reduce(kind, t, group):
    """dist.all_reduce(SUM) of a sync-BN statistics vector, with HIP events on the launch stream while bench.py profiles: the
    collective is stream-ordered on the compute stream's critical path, so event time = what it costs the step."""
    if PROFILE_COMM is None:
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
        return
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    e0.record(torch.cuda.current_stream())
    dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
    e1.record(torch.cuda.current_stream())
    PROFILE_COMM.append((kind, t.numel() * t.element_size(), e0, e1))


class role(object):
    """with ops.role('encoder_3x3'): ...   -- labels the forward conv launches issued inside (profiling only)."""

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        self.prev = _ROLE[0]; _ROLE[0] = self.name

    def __exit__(self, *a):
        _ROLE[0] = self.prev


class _hbm(object):
    """HIP events on the launch stream around one memory-bound stage (no-op unless bench.py profiles)."""

    def __init__(self, stage, nbytes):
        self.rec = PROFILE_HBM is not None
        if self.rec:
            self.stage, self.nbytes = stage, float(nbytes)
            self.e0 = torch.cuda.Event(enable_timing=True); self.e1 = torch.cuda.Event(enable_timing=True)

    def __enter__(self):
        if self.rec:
            self.e0.record(torch.cuda.current_stream())

    def __exit__(self, *a):
        if self.rec:
            self.e1.record(torch.cuda.current_stream())
            PROFILE_HBM.append((self.stage, self.nbytes, self.e0, self.e1))


_CONV_LABELS = {0: 'conv_igemm_kernel<128,128>', 1: 'conv_igemm_kernel<256,64>', 2: 'conv_igemm_kernel<256,32>',
                20: 'conv_igemm_dma_kernel<128,128>', 21: 'conv_igemm_dma_kernel<256,64>', 22: 'conv_igemm_dma_kernel<128,64>',
                30: 'conv_igemm_halo_kernel<128,128>', 31: 'conv_igemm_halo_kernel<256,64>', 32: 'conv_igemm_halo_kernel<128,64>',
                33: 'conv_igemm_halo16_kernel<128,128>', 34: 'conv_igemm_halo16_kernel<128,64>',
                40: 'conv_igemm_halo_x3_kernel<128,128>', 41: 'conv_igemm_halo_x3_kernel<128,64>',
                42: 'conv_igemm_halo_x3_kernel<128,64,4,1,true>', 50: 'conv_igemm_dma_x3_kernel<64>', 51: 'conv_igemm_dma_x3_kernel<128>',
                60: 'conv_halo_k32_kernel<8,128>', 61: 'conv_halo_k32_kernel<4,64>', 62: 'conv_halo_k32_kernel<16,64>',
                63: 'conv_halo_k32_kernel<8,16>', 64: 'conv_halo_k32_kernel<8,32>',
                10: 'thin_small_cout_kernel',
                12: 'thin4_cin_kernel', 13: 'thin4_cout_kernel', 14: 'tiny4_kernel', 15: 'thin32_cin_kernel', 16: 'conv1x1_k64_kernel'}
_WGRAD_LABELS = {0: 'wgrad_kernel<128,128>', 1: 'wgrad_kernel<128,64>', 2: 'wgrad_kernel<128,32>',
                 20: 'wgrad_dma_kernel<128,128>', 21: 'wgrad_dma_kernel<128,64>',
                 30: 'wgrad_halo_kernel<32,128>', 31: 'wgrad_halo_kernel<64,64>',
                 40: 'wgrad_halo_x3_kernel<32,128>', 41: 'wgrad_halo_x3_kernel<64,64>', 60: 'wgrad_k32_kernel<64,64>',
                 50: 'wgrad_dma_x3_kernel<128,128>', 51: 'wgrad_dma_x3_kernel<128,64>',
                 15: 'wgrad4_kernel<thin_cout>', 16: 'wgrad4_kernel<thin_cin>', 17: 'wgrad_tiny4_kernel', 18: 'wgrad32_cin_kernel'}


class _Timed(object):
    def __init__(self, label, flops, tag=None):
        self.rec = PROFILE is not None
        if self.rec:
            self.label, self.flops, self.tag = label, flops, tag
            self.e0 = torch.cuda.Event(enable_timing=True); self.e1 = torch.cuda.Event(enable_timing=True)

    def __enter__(self):
        if self.rec:
            self.e0.record(torch.cuda.current_stream())

    def __exit__(self, *a):
        if self.rec:
            self.e1.record(torch.cuda.current_stream())
            PROFILE.append((self.label, self.flops, self.e0, self.e1, self.tag))


_CONV_SHAPE = ' n%d %dx%d cin%d cout%d taps%d s%d/%d'      # n, GH, GW, Cin, Cout, taps, in stride, out stride
_WGRAD_SHAPE = ' n%d %dx%d cin%d cout%d k%d s%d'           # n, GH, GW, Cin, Cout, KH, stride
# how a launch is named while profiling: (label table, entry point that returns the kernel id, PROFILE_SHAPES text)
_CONV_KIND = (_CONV_LABELS, 'ssg_conv2d_kernel_id', _CONV_SHAPE)
_WGRAD_KIND = (_WGRAD_LABELS, 'ssg_conv2d_wgrad_kernel_id', _WGRAD_SHAPE)


def _timed_call(kind, entry, d, args, shape, flops, suffix='', tag=None):
    """call(entry, &d, *args, stream): one MFMA launch.  While PROFILE is a list it is timed under its kernel's label + suffix
    (+ the launch geometry `shape` under PROFILE_SHAPES); the id query is made only then."""
    label = None
    if PROFILE is not None:
        labels, id_entry, shape_fmt = kind
        label = labels.get(call(id_entry, C.byref(d)), '?') + suffix
        if PROFILE_SHAPES:
            label += shape_fmt % shape
    with _Timed(label, flops, tag):
        call(entry, C.byref(d), *args, stream_ptr())


class _Declined(Exception):
    """_conv_launch: the library has no kernel for this parity-merged / in_affine / bwd_stats launch (nothing was allocated or launched)."""


def _conv_launch(x1, x2, wpk, kp, kmode, row0, cout, bias, res, act, slope, taps, n, h, w, gh, gw, oh, ow,
                 in_s, out_s, out_oy, out_ox, out, want_bn=False, tag=None, parity_merge=False, in_affine=None, bwd_stats=None):
    """Returns None, or -- with want_bn and a kernel that has the statistics epilogue -- the fp64 tensor [rows, 2, cout] of
    per-tile (sum, sum of squares) of the conv output (ssg_conv_desc.bnpart).  parity_merge: the nine taps are the four parity
    classes of a 3x3 stride-2 input gradient (ssg_conv_desc.parity_merge).  in_affine = (scale[C1], shift[C1], act, slope): the
    launch convolves act(x1 * scale + shift) (ssg_conv_desc.in_scale: a batch-norm apply that is never materialised).
    bwd_stats = (x, stats rows [mean, invstd, scale, shift], act, slope): the launch produces d(act(bn(x))), masks it and writes the
    batch-norm backward sums as per-tile rows (ssg_conv_desc.bwd_x).  Raises _Declined, with nothing allocated or launched, where
    the library has no kernel for a parity_merge / in_affine / bwd_stats launch."""
    d = _conv_desc(_at(x1), pad4(x1.shape[1]), _at(x2) if x2 is not None else None, pad4(x2.shape[1]) if x2 is not None else 0,
                   (n, h, w), wpk.data_ptr() + row0 * kp * 4, kp, kmode, bias, _at(res) if res is not None else None, _at(out), cout,
                   (gh, gw, oh, ow), in_s, out_s, (out_oy, out_ox), taps, act, slope)
    d.parity_merge = 1 if parity_merge else 0
    pack = call('ssg_conv2d_split_bn', C.byref(d)) if MFMA_SPLIT and kmode == 0 else 0
    if parity_merge and pack != 64:
        raise _Declined()
    d.w_split = 1 if pack else None         # placeholder until the pack exists: the queries below depend on the kernel it selects
    if in_affine is not None:
        d.in_scale = in_affine[0].data_ptr(); d.in_shift = in_affine[1].data_ptr(); d.in_act = int(in_affine[2]); d.in_slope = float(in_affine[3])
        if not call('ssg_conv2d_in_affine_ok', C.byref(d)):
            raise _Declined()
    if bwd_stats is not None:
        bx, bst, bact, bslope = bwd_stats
        d.bwd_x = bx.data_ptr(); d.bwd_ldx = _ld(bx); d.bwd_scale = bst[2].data_ptr(); d.bwd_shift = bst[3].data_ptr()
        d.bwd_mean = bst[0].data_ptr(); d.bwd_act = int(bact); d.bwd_slope = float(bslope)
        if not call('ssg_conv2d_bwd_stats_ok', C.byref(d)):
            raise _Declined()
        want_bn = True
    rows = call('ssg_conv2d_bnpart_rows', C.byref(d)) if want_bn else 0
    if bwd_stats is not None and rows == 0:
        raise _Declined()
    split = _split_pack(wpk, row0, cout, kp, pack) if pack else None
    d.w_split = split.data_ptr() if split is not None else None
    part = None
    if rows > 0:
        part = torch.empty((rows, 2, cout), dtype=torch.float64, device=out.device)
        d.bnpart = part.data_ptr()
    ws = None
    if part is None and split is None:  # split-K (small pixel grids with a long reduction): the kernel needs a workspace
        need = call('ssg_conv2d_workspace_bytes', C.byref(d))
        if need > 0:
            ws = _ws(need, out.device)
            d.ws = ws.data_ptr(); d.ws_bytes = need
    cred = x1.shape[1] + (x2.shape[1] if x2 is not None else 0)
    _timed_call(_CONV_KIND, 'ssg_conv2d_f32', d, (), (n, gh, gw, cred, cout, len(taps), in_s, out_s),
                2.0 * n * gh * gw * cout * cred * len(taps), '+splitk' if ws is not None else '', tag)
    return part


import os as _os
# The dense 3x3 unit-stride convs and their input gradients multiply on the bf16 matrix pipe with every fp32 operand split into
# three bf16 terms (csrc/conv_igemm_halo_x3.hip: the error against fp64 is that of the fp32-MFMA kernel, tests/test_split_gpu.py;
# 16/6 of the fp32 MFMA rate).  SSG_MFMA_SPLIT=0 keeps them on v_mfma_f32_32x32x2_f32 (conv_igemm_halo.hip).
MFMA_SPLIT = _os.environ.get('SSG_MFMA_SPLIT', '1') == '1'
# SSG_BN_FUSE_INPUT=1: relu(bn1(conv1(x))) of a residual block is applied on conv2's input (and on the x operand of conv2's weight
# gradient) instead of being written out -- same bits (tests/test_blocks_gpu.py), one activation less to keep, 1.0 ms less in the
# batch-norm passes of the 16 x 512^2 step and 1.0-2.5 ms MORE in the k32 kernels that take the transform (issue-bound: the extra
# vector work on the operand path is not hidden), same-box A/B 195.5-195.9 vs 195.8-197.4 ms.  Off by default.
BN_FUSE_INPUT = _os.environ.get('SSG_BN_FUSE_INPUT', '0') == '1'
# SSG_PARITY_MERGE=0: the input gradient of a 3x3 stride-2 conv as four launches (one per output parity class) again
PARITY_MERGE = _os.environ.get('SSG_PARITY_MERGE', '1') != '0'


def _split_pack(wpk, row0, rows, kp, bn):
    """bf16x3 split of rows [row0, row0 + rows) of a packed fp32 weight matrix for column tile `bn` (cached on the packed
    tensor, which itself lives in the parameter's pack cache: both go stale together)."""
    cache = wpk.__dict__.get('_ssg_split')
    if cache is None:
        cache = _attach(wpk, '_ssg_split', {})
    key = (row0, rows, bn)
    hit = cache.get(key)
    if hit is None:
        nbytes = call('ssg_pack_weights_split_bytes', rows, kp, bn)
        hit = torch.empty(nbytes // 2, dtype=torch.int16, device=wpk.device)
        call('ssg_pack_weights_split_bf16x3', wpk.data_ptr() + row0 * kp * 4, rows, kp, bn, ptr(hit), stream_ptr())
        cache[key] = hit
    return hit


def _out_size(h, k, s, p):
    return (h + 2 * p - k) // s + 1


def _out_hw(h, w, kh, kw, s, pad):
    pt, pb, pl, pr = _pad4(pad)
    return (h + pt + pb - kh) // s + 1, (w + pl + pr - kw) // s + 1


def _x1_routed(precision, stride, pad, wscale, fused):
    """True where a conv call under `precision` asks the bf16x1 / bf16x2 kernels first: 'bf16x1' or 'bf16x2' (which of the two
    families: the string itself) and a unit-stride pad-1 conv of unscaled
    weights (the 3x3 window and the shapes are the launchers' own predicates).  `fused` (in_affine / bwd_stats) has no bf16x1
    form: the combination is refused."""
    if precision == 'fp32':
        return False
    if precision not in ('bf16x1', 'bf16x2'):
        raise ValueError('conv: unknown precision %r (one of %s)' % (precision, ', '.join(_PRECISIONS)))
    if fused is not None:
        raise ValueError("conv: in_affine / bwd_stats cannot be combined with precision=%r" % (precision,))
    return stride == 1 and _pad4(pad) == (1, 1, 1, 1) and wscale is None


def _x1_s2_routed(precision, x1_s2, stride, pad, wscale):
    """True where a call from the single-conv node (`x1_s2`: _Conv2d passes it, the block nodes never do) under 'bf16x1' asks the
    stride-2 bf16x1 kernels first: a stride-2 pad-1 conv of unscaled weights."""
    return bool(x1_s2) and precision == 'bf16x1' and stride == 2 and _pad4(pad) == (1, 1, 1, 1) and wscale is None


def _conv_fwd_impl(x1, x2, weight, bias, stride, pad, act, slope, res=None, out=None, wscale=None, want_bn=False, in_affine=None, precision='fp32',
                   x1_s2=False):
    """Returns y, or (y, part) with want_bn: part = per-tile batch-norm partial sums of y from the conv epilogue, or None when
    the kernel this shape maps to has none (the batch norm then runs its own statistics pass).  in_affine: see _conv_launch; the
    result is None (nothing launched) when the library declines.  precision='bf16x1': a unit-stride 3x3 pad-1 conv runs on
    _conv_bf16x1_impl where conv2d_bf16x1_ok holds (part is then None: that launcher has no statistics epilogue) and on the
    fp32-class kernel below where it refuses.  x1_s2 (the single-conv node only): a 3x3 stride-2 pad-1 conv without x2 / res asks
    _conv_s2_bf16x1_impl first in the same way.  precision='bf16x2': the same routing to the two-term kernel
    (csrc/conv_halo_k32_bf16.hip) for the unit-stride conv; stride 2 stays fp32-class."""
    if _x1_routed(precision, stride, pad, wscale, in_affine) and conv2d_bf16x1_ok(x1, weight, x2=x2, res=res, family=precision):
        y = _conv_bf16x1_impl(x1, weight, bias, act, slope, x2=x2, res=res, out=out, family=precision)
        return (y, None) if want_bn else y
    if _x1_s2_routed(precision, x1_s2, stride, pad, wscale) and x2 is None and res is None and in_affine is None:
        y = _conv_s2_bf16x1_impl(x1, weight, bias, act, slope, out=out)
        if y is not None:
            return (y, None) if want_bn else y
    o, i, kh, kw = weight.shape
    n, c1, h, w = x1.shape
    c2 = x2.shape[1] if x2 is not None else 0
    if x2 is not None and c1 % 4:
        raise ValueError('two-input conv needs C1 %% 4 == 0 (got %d)' % c1)
    if c1 + c2 != i:
        raise ValueError('conv: input channels %d+%d != weight in-channels %d' % (c1, c2, i))
    cred_pad = pad4(c1) + pad4(c2)
    taps = _taps_fwd(kh, kw, pad)
    wpk, kp, kmode = _pack(weight, 0, taps, cred_pad, pad4(c1), sigma=wscale)
    oh, ow = _out_hw(h, w, kh, kw, stride, pad)
    if out is None:
        out = new_nhwc(n, o, oh, ow, x1.device)
    try:
        part = _conv_launch(x1, x2, wpk, kp, kmode, 0, o, bias, res, act, slope, taps, n, h, w, oh, ow, oh, ow, stride, 1, 0, 0, out,
                            want_bn=want_bn and res is None and act == ACT_NONE,
                            tag=_ROLE[0] if (kh == 3 and kw == 3 and _ROLE[0] is not None) else None, in_affine=in_affine)
    except _Declined:
        return None
    return (out, part) if want_bn else out


def _conv_dgrad_impl(dy, weight, stride, pad, h, w, c_lo, c_hi, res=None, wscale=None, bwd_stats=None, precision='fp32', x1_s2=False):
    """Input gradient for input channels [c_lo, c_hi) -> NHWC tensor [N, c_hi-c_lo, h, w].
    `res` (same shape) is added in the epilogue: gradient accumulation without an extra pass.
    bwd_stats = (x, stats, act, slope): the gradient is that of act(bn(x)); returns (g, part) -- the MASKED gradient and the per-tile rows
    (sum g, sum g * (x - mean)) of the batch-norm backward from the epilogue (ssg_conv_desc.bwd_x) -- or None, with nothing launched,
    where the kernel this launch maps to has no such epilogue.  precision='bf16x1': a unit-stride 3x3 pad-1 gradient is
    _conv_dgrad_bf16x1_impl's where that takes it, and the fp32-class kernel's below where it refuses.  x1_s2 (the single-conv node
    only): a 3x3 stride-2 pad-1 gradient without res is _conv_dgrad_s2_bf16x1_impl's where all four parity classes are legal."""
    if _x1_routed(precision, stride, pad, wscale, bwd_stats):
        dx = _conv_dgrad_bf16x1_impl(dy, weight, h, w, c_lo, c_hi, res=res, family=precision)
        if dx is not None:
            return dx
    if _x1_s2_routed(precision, x1_s2, stride, pad, wscale) and res is None and bwd_stats is None:
        dx = _conv_dgrad_s2_bf16x1_impl(dy, weight, h, w, c_lo, c_hi)
        if dx is not None:
            return dx
    o, i, kh, kw = weight.shape
    n, _, oh, ow = dy.shape
    cred_pad = pad4(o)
    pt, _, pl, _ = _pad4(pad)
    dx = new_nhwc(n, c_hi - c_lo, h, w, dy.device)
    if stride == 1:
        taps = [(ky, kx, pt - ky, pl - kx) for ky in range(kh) for kx in range(kw)]
        wpk, kp, kmode = _pack(weight, 1, taps, cred_pad, cred_pad, sigma=wscale)
        try:
            part = _conv_launch(dy, None, wpk, kp, kmode, c_lo, c_hi - c_lo, None, res, ACT_NONE, 0.0, taps, n, oh, ow, h, w, h, w, 1, 1, 0, 0,
                                dx, bwd_stats=bwd_stats)
        except _Declined:
            return None
        return dx if bwd_stats is None else (dx, part)
    if bwd_stats is not None:
        return None
    if res is not None:
        raise NotImplementedError('strided dgrad with fused accumulation')
    s = stride
    classes = []
    for py in range(s):
        for px in range(s):
            taps = [(ky, kx, (py + pt - ky) // s, (px + pl - kx) // s) for ky in range(kh) for kx in range(kw)
                    if (py + pt - ky) % s == 0 and (px + pl - kx) % s == 0]
            classes.append((py, px, taps))
    # eligibility of the merged launch is decided BEFORE its 9-tap pack is built: the library declines dy narrower
    # than 17 pixels, channel counts that are not whole 64-column tiles and tensors beyond 32-bit byte offsets
    # (ssg_conv_halo_x3_parity_ok); with spectral norm a declined pack would be an uncached launch + allocation per backward
    if (PARITY_MERGE and s == 2 and kh == 3 and kw == 3 and (pt, pl) == (1, 1) and MFMA_SPLIT and ow >= 17
            and (c_hi - c_lo) % 64 == 0 and dy.numel() * 4 <= 0xfffffff0):
        # the four classes read the same 2x2 neighbourhood of dy: one launch, nine tap steps, four accumulator sets
        # (conv_igemm_halo_x3_kernel<..., PARITY>); falls through to the per-class launches where the library declines
        merged = [t for _, _, taps in classes for t in taps]
        wpk, kp, kmode = _pack(weight, 1, merged, cred_pad, cred_pad, sigma=wscale)
        try:
            _conv_launch(dy, None, wpk, kp, kmode, c_lo, c_hi - c_lo, None, None, ACT_NONE, 0.0, merged, n, oh, ow,
                         (h + 1) // 2, (w + 1) // 2, h, w, 1, s, 0, 0, dx, parity_merge=True)
            return dx
        except _Declined:
            pass
    if any(len(t) == 0 for _, _, t in classes):
        # no launch writes the pixels of a class without taps: fill the whole buffer, pad lanes included (dx.zero_() on the
        # logical view left lane 3 of a 3-channel gradient unwritten)
        _relabel(dx, _ld(dx)).zero_()
    for py, px, taps in classes:
        gh, gw = (h - py + s - 1) // s, (w - px + s - 1) // s
        if not taps or gh <= 0 or gw <= 0:
            continue
        wpk, kp, kmode = _pack(weight, 1, taps, cred_pad, cred_pad, sigma=wscale)
        _conv_launch(dy, None, wpk, kp, kmode, c_lo, c_hi - c_lo, None, None, ACT_NONE, 0.0, taps, n, oh, ow, gh, gw, h, w, 1, s, py, px, dx)
    return dx


def _check_wgrad_s2(who, precision, wgrad_s2):
    """The second switch's values: 'fp32' | 'bf16x1', the latter only beside precision='bf16x1' (there is no two-term stride-2
    weight gradient: 'bf16x2' is not a value of this switch, and precision='bf16x2' takes wgrad_s2='fp32' only)."""
    if wgrad_s2 not in ('fp32', 'bf16x1'):
        raise ValueError('%s: unknown wgrad_s2 %r (one of fp32, bf16x1)' % (who, wgrad_s2))
    if wgrad_s2 == 'bf16x1' and precision != 'bf16x1':
        raise ValueError("%s: wgrad_s2='bf16x1' needs precision='bf16x1' (got %r)" % (who, precision))


def _conv_wgrad_impl(x1, x2, dy, weight_shape, stride, pad, in_affine=None, precision='fp32', wgrad_s2='fp32'):
    """in_affine = (scale, shift, act, slope): the x operand is act(x1 * scale + shift) (ssg_wgrad_desc.in_scale); returns None,
    with nothing launched, when the kernel this shape maps to has no such transform.  precision='bf16x1': a unit-stride 3x3 pad-1
    weight gradient is _conv_wgrad_bf16x1_impl's where that takes it, and the fp32-class kernel's below where it refuses.
    wgrad_s2='bf16x1' (beside precision='bf16x1' only; the single-conv node passes it, the block nodes never do): a 3x3 stride-2
    pad-1 weight gradient without x2 / in_affine is _conv_wgrad_s2_bf16x1_impl's where that takes it."""
    if _x1_routed(precision, stride, pad, None, in_affine):
        dw = _conv_wgrad_bf16x1_impl(x1, x2, dy, weight_shape, family=precision)
        if dw is not None:
            return dw
    if (precision == 'bf16x1' and wgrad_s2 == 'bf16x1' and stride == 2 and _pad4(pad) == (1, 1, 1, 1) and x2 is None
            and in_affine is None):
        dw = _conv_wgrad_s2_bf16x1_impl(x1, dy, weight_shape)
        if dw is not None:
            return dw
    o, i, kh, kw = weight_shape
    n = x1.shape[0]
    _, _, oh, ow = dy.shape
    d = _wgrad_desc(x1, pad4(x1.shape[1]), x2, pad4(x2.shape[1]) if x2 is not None else 0, dy, weight_shape, stride,
                    _taps_fwd(kh, kw, pad))
    dw = torch.empty((o, i, kh, kw), device=dy.device, dtype=torch.float32)
    d.dw_oihw = dw.data_ptr()
    d.flags = 1 if MFMA_SPLIT else 0
    if in_affine is not None:
        d.in_scale = in_affine[0].data_ptr(); d.in_shift = in_affine[1].data_ptr(); d.in_act = int(in_affine[2]); d.in_slope = float(in_affine[3])
        if not call('ssg_conv2d_wgrad_in_affine_ok', C.byref(d)):
            return None
    nbytes = call('ssg_conv2d_wgrad_workspace_bytes', C.byref(d))
    ws = _ws(nbytes, dy.device)
    d.ws = ws.data_ptr(); d.ws_bytes = ws.numel() * 8
    _timed_call(_WGRAD_KIND, 'ssg_conv2d_wgrad_f32', d, (), (n, oh, ow, i, o, kh, stride), 2.0 * n * oh * ow * o * i * kh * kw)
    return dw


def _channel_sum(x, c):
    n, _, h, w = x.shape
    p = n * h * w
    out = torch.empty(c, device=x.device, dtype=torch.float32)
    ws = _ws(call('ssg_bn_workspace_bytes', p, c), x.device)
    call('ssg_channel_sum_f32', ptr(x), p, c, _ld(x), ptr(out), ptr(ws), stream_ptr())
    return out


def _act_bwd(y, dy, act, slope):
    n, c, h, w = y.shape
    dx = new_nhwc(n, c, h, w, y.device)
    call('ssg_act_bwd_f32', ptr(y), _ld(y), ptr(dy), _ld(dy), n * h * w, pad4(c), act, slope, ptr(dx), _ld(dx), stream_ptr())
    return dx


class _Conv2d(torch.autograd.Function):
    """F.conv2d (+bias, +activation, optional second input = channel concat) on MFMA.  `precision` (see _conv_fwd_impl) is the
    forward's and, kept on ctx, that of the three gradients.  This node, and no other, also asks the stride-2 bf16x1 kernels
    (x1_s2) under 'bf16x1', and the stride-2 bf16x1 weight gradient where `wgrad_s2` (kept on ctx beside it) says so."""

    @staticmethod
    def forward(ctx, x1, x2, weight, bias, stride, pad, act, slope, res=None, want_bn=False, precision='fp32', wgrad_s2='fp32'):
        ctx.set_materialize_grads(False)       # no zero tensor for the (non-differentiable) statistics output's gradient
        x1 = to_nhwc(x1)
        x2 = to_nhwc(x2) if x2 is not None else None
        res = to_nhwc(res) if res is not None else None
        r = _conv_fwd_impl(x1, x2, weight, bias, stride, pad, act, slope, res=res, want_bn=want_bn, precision=precision, x1_s2=True)
        y, part = r if want_bn else (r, None)
        ctx.cfg = (stride, pad, act, slope, precision, wgrad_s2)
        ctx.save_for_backward(x1, x2, weight, y if act != ACT_NONE else None)
        ctx.has_bias = bias is not None
        ctx.has_res = res is not None
        if part is None:
            part = torch.empty(0, dtype=torch.float64, device=y.device)
        ctx.mark_non_differentiable(part)
        return y, part

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy, _=None):
        if dy is None:
            return (None,) * 12
        x1, x2, weight, y = ctx.saved_tensors
        stride, pad, act, slope, precision, wgrad_s2 = ctx.cfg
        dy = to_nhwc(dy)
        n, c1, h, w = x1.shape
        dx1 = dx2 = dw = db = None
        want_db = ctx.has_bias and ctx.needs_input_grad[3]
        cout = weight.shape[0]
        if (act in (ACT_RELU, ACT_LRELU) and want_db and cout % 4 == 0 and dy.shape[1] == cout and dy.dtype == torch.float32
                and _bn_lean()):
            # activation backward and bias gradient in one sweep over dy (the discriminator's stem): the masked gradient is written
            # while its column sums are carried, instead of _act_bwd and a _channel_sum pass over what it wrote -- same bits
            dy, _, sums = _frozen_bwd(None, y, dy, None, None, None, None, act, slope)
            db = sums[:cout].float()
        elif act != ACT_NONE:
            dy = _act_bwd(y, dy, act, slope)
        if ctx.needs_input_grad[0]:
            dx1 = _conv_dgrad_impl(dy, weight, stride, pad, h, w, 0, c1, precision=precision, x1_s2=True)
        if x2 is not None and ctx.needs_input_grad[1]:
            dx2 = _conv_dgrad_impl(dy, weight, stride, pad, h, w, c1, c1 + x2.shape[1], precision=precision, x1_s2=True)
        if ctx.needs_input_grad[2]:
            dw = _conv_wgrad_impl(x1, x2, dy, weight.shape, stride, pad, precision=precision, wgrad_s2=wgrad_s2)
        if want_db and db is None:
            db = _channel_sum(dy, cout)
        dres = dy if (ctx.has_res and ctx.needs_input_grad[8]) else None      # residual joins before the activation
        return dx1, dx2, dw, db, None, None, None, None, dres, None, None, None


def conv2d(x, weight, bias=None, stride=1, padding=0, act=ACT_NONE, slope=0.0, x2=None, res=None, bn_stats=False, precision='fp32',
           wgrad_s2='fp32'):
    """F.conv2d on the HIP kernels.  `padding`: int or (top, bottom, left, right) (TF-"same" static
    padding of the EfficientNet convs is asymmetric); `x2`: second tensor concatenated after x;
    `res`: tensor added in the epilogue before the activation (act(conv(x) + bias + res)).
    `bn_stats=True`: returns (y, part) -- `part` are the per-tile (sum, sum of squares) of y from the conv epilogue (empty when
    this shape's kernel has none); hand it to batch_norm_act(y, bn, stats_part=part) to skip its statistics pass.
    `precision='bf16x1'` (opt-in, an approximation: both operands rounded once to bf16, fp32 accumulation): a 3x3 pad-1 conv of
    stride 1 or 2 asks the one-term kernels first, in the forward and in each of its gradients, and runs today's kernel wherever
    their predicates refuse -- it never raises for a shape; `part` of a routed forward is empty.  'fp32' (default): today's launches.
    `wgrad_s2='bf16x1'` (opt-in beside precision='bf16x1', ValueError otherwise): the weight gradient of a 3x3 stride-2 pad-1 conv
    asks the one-term stride-2 kernel first as well; 'fp32' (default) leaves it on today's kernel.
    `precision='bf16x2'` (opt-in, an approximation ~2^8 times tighter than 'bf16x1': each operand split into two bf16 terms, the
    three largest products kept, |error| <= (3 * 2^-16 + 3 * 2^-32) * conv(|x|, |w|) plus fp32 accumulation): a 3x3 pad-1 conv of
    stride 1 asks the two-term kernels first in the forward and in each gradient, and runs today's kernel where they refuse;
    stride 2 stays on today's kernels."""
    _lib.require_gpu(x)
    if precision not in _PRECISIONS:
        raise ValueError('conv2d: unknown precision %r (one of %s)' % (precision, ', '.join(_PRECISIONS)))
    _check_wgrad_s2('conv2d', precision, wgrad_s2)
    weight = param('conv2d', 'weight', weight, x, packed=True)
    bias = param('conv2d', 'bias', bias, x)
    pad = tuple(int(v) for v in padding) if isinstance(padding, (tuple, list)) else int(padding)
    y, part = _Conv2d.apply(x, x2, weight, bias, int(stride), pad, int(act), float(slope), res, bool(bn_stats), precision, wgrad_s2)
    return (y, part) if bn_stats else y


# ----------------------------------------------------------------------------- opt-in bf16 inference convolution
# csrc/conv_halo_k32_bf16.hip: the 3x3 stride-1 pad-1 forward conv with both operands rounded once to bf16 and one MFMA per product
# (ssg_conv2d_bf16x1_f32).  An approximation, forward only, chosen per call: nothing here is reached from a training path, and
# ops.conv2d never routes to it.
_X1_LABELS = {70: 'conv_halo_k32_x1_kernel<128>', 71: 'conv_halo_k32_x1_kernel<64>'}
_X1_KIND = (_X1_LABELS, 'ssg_conv2d_bf16x1_kernel_id', _CONV_SHAPE)
_X1_TAPS = _taps_fwd(3, 3, 1)
_PRECISIONS = ('fp32', 'bf16x1', 'bf16x2')
# csrc/conv_halo_k32_bf16.hip / conv_wgrad_k32_bf16.hip: the two-term kernels behind precision='bf16x2', same descriptors and call
# shapes as the one-term ones.  A family = the entry-point infix, its label tables and the cache attribute of its weight packs.
_X2_LABELS = {90: 'conv_halo_k32_x2_kernel<128>', 91: 'conv_halo_k32_x2_kernel<64>'}
_X2_KIND = (_X2_LABELS, 'ssg_conv2d_bf16x2_kernel_id', _CONV_SHAPE)
_WGRAD_X2_LABELS = {92: 'wgrad_k32_x2_kernel'}
_WGRAD_X2_KIND = (_WGRAD_X2_LABELS, 'ssg_conv2d_wgrad_bf16x2_kernel_id', _WGRAD_SHAPE)


def _x_kind(family):
    return _X2_KIND if family == 'bf16x2' else _X1_KIND


class _precision(object):
    """Base of infer_precision / train_precision: a nestable context that sets its own class's mode (`_state`)."""

    def __init__(self, mode):
        if mode not in _PRECISIONS:
            raise ValueError('%s: unknown mode %r (one of %s)' % (type(self).__name__, mode, ', '.join(_PRECISIONS)))
        self.mode = mode

    def __enter__(self):
        self.prev = self._state[0]; self._state[0] = self.mode
        return self

    def __exit__(self, *a):
        self._state[0] = self.prev


class infer_precision(_precision):
    """with ops.infer_precision('bf16x1'): ...   -- eval-mode modules (archs.BasicBlock) run their 3x3 stride-1 convs on
    conv2d_bf16x1 where conv2d_bf16x1_ok holds (bf16 operand rounding, fp32 accumulation: an approximation) and stay on conv2d
    elsewhere.  'fp32' (the default) is today's behaviour.  Read by eval-mode module code under torch.no_grad() only: a forward
    that records a graph (autograd enabled and something requires grad) runs the fp32-class kernels whatever the mode says, and so
    does every training path.  'bf16x2': the same convs through conv2d(precision='bf16x2') -- two bf16 terms per operand, three
    products (conv_halo_k32_x2_kernel), per-launch fallback to the fp32-class kernel where ssg_conv2d_bf16x2_ok declines."""
    _state = ['fp32']


def infer_precision_mode():
    """The mode the innermost `infer_precision` block set ('fp32' outside any)."""
    return infer_precision._state[0]


def _x1_desc(x, x2, weight, res, out=None):
    """ssg_conv_desc of conv2d_bf16x1 for these tensors.  Pointers the predicate does not dereference (the packed weights, an
    output that does not exist yet, a tensor that to_nhwc would still copy) are stood in for by an aligned non-null value."""
    def side(t):
        ld = nhwc_ld(t)
        return (t.data_ptr(), ld) if ld is not None else (16, pad4(t.shape[1]))
    n, c1, h, w = x.shape
    c2 = x2.shape[1] if x2 is not None else 0
    o = weight.shape[0]
    return _conv_desc(side(x), c1, side(x2) if x2 is not None else None, c2, (n, h, w), 16, 9 * (c1 + c2), 0, None,
                      side(res) if res is not None else None, side(out) if out is not None else (16, pad4(o)), o,
                      (h, w, h, w), 1, 1, (0, 0), _X1_TAPS, ACT_NONE, 0.0)


def _x1_shapes_ok(x, weight, x2, res):
    if x.dim() != 4 or weight.dim() != 4 or tuple(weight.shape[2:]) != (3, 3) or x.dtype != torch.float32 or weight.dtype != torch.float32:
        return False
    c2 = x2.shape[1] if x2 is not None else 0
    if x.shape[1] + c2 != weight.shape[1] or (x2 is not None and (x2.dtype != torch.float32 or x2.shape[0] != x.shape[0] or x2.shape[2:] != x.shape[2:])):
        return False
    return res is None or (res.dtype == torch.float32 and tuple(res.shape) == (x.shape[0], weight.shape[0], x.shape[2], x.shape[3]))


def conv2d_bf16x1_ok(x, weight, x2=None, res=None, family='bf16x1'):
    """True where conv2d_bf16x1 takes these tensors (ssg_conv2d_bf16x1_ok): a 3x3 weight, C1 % 32 == 0 and C2 % 32 == 0,
    Cout % 64 == 0, W >= 17, fp32 tensors below 4 GiB.  Launches nothing."""
    if not _x1_shapes_ok(x, weight, x2, res):
        return False
    return call('ssg_conv2d_%s_ok' % family, C.byref(_x1_desc(x, x2, weight, res))) != 0


def conv2d_bf16x2_ok(x, weight, x2=None, res=None):
    """True where conv2d(..., precision='bf16x2') runs its forward on the two-term kernel (ssg_conv2d_bf16x2_ok): the shapes of
    conv2d_bf16x1_ok.  Launches nothing."""
    return conv2d_bf16x1_ok(x, weight, x2=x2, res=res, family='bf16x2')


def _x1_pack(weight, wpk, kp, fmt, transpose=0, row0=0, rows=None, family='bf16x1'):
    """The bf16 pack of `weight` (OIHW) for format `fmt`, built from its fp32 kmode-0 matrix `wpk`; cached on the weight tensor as
    `_ssg_pack_bf16x1`, stamped like `_ssg_pack`.  transpose / row0 / rows: rows [row0, row0 + rows) of the TRANSPOSED matrix (an
    input gradient for a channel slice of a concat input); such packs are keyed (transpose, row0, rows, fmt)."""
    cache = _stamped_cache(weight, '_ssg_pack_' + family)           # family 'bf16x2': `_ssg_pack_bf16x2`, format codes 2128 / 2064
    if rows is None:
        rows = weight.shape[0]
    key = (transpose, row0, rows, fmt) if transpose else fmt
    hit = cache.get(key)
    if hit is None:
        nbytes = call('ssg_pack_weights_%s_bytes' % family, rows, kp, fmt)
        hit = torch.empty(nbytes // 2, dtype=torch.int16, device=weight.device)
        call('ssg_pack_weights_' + family, wpk.data_ptr() + row0 * kp * 4, rows, kp, fmt, ptr(hit), stream_ptr())
        cache[key] = hit
    return hit


def _conv_bf16x1_impl(x, weight, bias, act, slope, x2=None, res=None, out=None, family='bf16x1'):
    """conv2d_bf16x1 after its argument checks; `out`: an NHWC destination (a channel slice of a wider buffer in the layout tests)."""
    x = to_nhwc(x.detach())
    x2 = to_nhwc(x2.detach()) if x2 is not None else None
    res = to_nhwc(res.detach()) if res is not None else None
    n, c1, h, w = x.shape
    o = weight.shape[0]
    wpk, kp, kmode = _pack(weight, 0, _X1_TAPS, weight.shape[1], c1)
    if out is None:
        out = new_nhwc(n, o, h, w, x.device)
    d = _x1_desc(x, x2, weight, res, out)
    d.w = wpk.data_ptr(); d.Kp = kp; d.kmode = kmode
    d.bias = bias.data_ptr() if bias is not None else None
    d.act = int(act); d.slope = float(slope)
    fmt = call('ssg_conv2d_%s_ok' % family, C.byref(d))
    if not fmt:
        call('ssg_conv2d_%s_f32' % family, C.byref(d), None, stream_ptr())      # refused on the host, nothing launched: raises with the reason
    pack = _x1_pack(weight, wpk, kp, fmt, family=family)
    _timed_call(_x_kind(family), 'ssg_conv2d_%s_f32' % family, d, (ptr(pack),), (n, h, w, weight.shape[1], o, 9, 1, 1),
                2.0 * n * h * w * o * weight.shape[1] * 9, tag=_ROLE[0])
    return out


def conv2d_bf16x1(x, weight, bias=None, act=ACT_NONE, slope=0.0, x2=None, res=None):
    """act(conv3x3(cat(x, x2), weight, stride 1, padding 1) + bias + res) with x, x2 and weight rounded once to bf16 (round to
    nearest even) and fp32 accumulation: one sixth of the matrix instructions of the fp32-class kernel behind `conv2d`.
    An APPROXIMATION, |error| <= (2^-8 + 2^-18) * conv(|x|, |w|); bias, res and the output are fp32.  Inference only: raises
    RuntimeError when autograd is recording and an argument requires grad, ValueError where `conv2d_bf16x1_ok` says no, and there
    is no CPU fallback."""
    _lib.require_gpu(x)
    weight = param('conv2d_bf16x1', 'weight', weight, x, packed=True)
    bias = param('conv2d_bf16x1', 'bias', bias, x)
    for t in (x2, res):
        if t is not None:
            _lib.require_gpu(t)
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, weight, bias, x2, res)):
        raise RuntimeError('conv2d_bf16x1 is inference-only (no backward): call it under torch.no_grad() or on tensors that do not require grad')
    if not conv2d_bf16x1_ok(x, weight, x2=x2, res=res):
        raise ValueError('conv2d_bf16x1: no bf16x1 kernel for x %s x2 %s weight %s res %s (conv2d_bf16x1_ok is False)' % (
            tuple(x.shape), None if x2 is None else tuple(x2.shape), tuple(weight.shape), None if res is None else tuple(res.shape)))
    return _conv_bf16x1_impl(x, weight, bias, act, slope, x2=x2, res=res)


# ----------------------------------------------------------------------------- opt-in bf16x1 training
# 'fp32 master weights, bf16 operands, fp32 accumulation' for the dense 3x3 stride-1 convs: forward and input gradient on
# conv_halo_k32_x1_kernel (the input gradient is the same convolution on dy with the transposed pack and the taps (1 - ky, 1 - kx)),
# weight gradient on wgrad_k32_x1_kernel (csrc/conv_wgrad_k32_bf16.hip).  Every tensor in HBM stays fp32.  Chosen by the caller:
# ops.conv2d never comes here.
_WGRAD_X1_LABELS = {72: 'wgrad_k32_x1_kernel'}
_WGRAD_X1_KIND = (_WGRAD_X1_LABELS, 'ssg_conv2d_wgrad_bf16x1_kernel_id', _WGRAD_SHAPE)
_X1_TAPS_T = [(ky, kx, 1 - ky, 1 - kx) for ky in range(3) for kx in range(3)]


class train_precision(_precision):
    """with ops.train_precision('bf16x1'): ...   -- autograd nodes that have a bf16x1 route (blocks._BasicBlockFn,
    blocks._FrozenBasicBlockFn) run their 3x3 stride-1 convs, forward, input gradient and weight gradient, with both operands
    rounded once to bf16 (fp32 accumulation, fp32 tensors: an approximation) wherever the kernels' predicates hold, and stay on the
    fp32-class kernels elsewhere.  models_seg_gan.ConvolutionalBlock (the discriminator) hands the mode to conv2d(precision=), whose
    node also has the stride-2 routes.  'fp32' (the default) launches exactly what runs without the context.  A node reads the mode in
    its forward and keeps it: its backward uses the forward's mode whatever is set when .backward() runs.
    wgrad_s2='bf16x1' (a second switch, default 'fp32', only beside mode 'bf16x1'): ConvolutionalBlock also hands this on, and the
    weight gradient of its stride-2 convs asks wgrad_s2_k32_x1_kernel first.  The block nodes do not read it.
    'bf16x2': the same nodes and launches on the two-term kernels (conv_halo_k32_x2_kernel, wgrad_k32_x2_kernel: each operand split
    into two bf16 terms, three products kept); stride-2 convs stay fp32-class and wgrad_s2 must stay 'fp32'."""
    _state = ['fp32']
    _s2_state = ['fp32']

    def __init__(self, mode, wgrad_s2='fp32'):
        super(train_precision, self).__init__(mode)
        _check_wgrad_s2('train_precision', mode, wgrad_s2)
        self.wgrad_s2 = wgrad_s2

    def __enter__(self):
        self.prev_s2 = self._s2_state[0]; self._s2_state[0] = self.wgrad_s2
        return super(train_precision, self).__enter__()

    def __exit__(self, *a):
        self._s2_state[0] = self.prev_s2
        return super(train_precision, self).__exit__(*a)


def train_precision_mode():
    """The mode the innermost `train_precision` block set ('fp32' outside any)."""
    return train_precision._state[0]


def train_wgrad_s2_mode():
    """The wgrad_s2 switch the innermost `train_precision` block set ('fp32' outside any)."""
    return train_precision._s2_state[0]


def _conv_wgrad_bf16x1_impl(x1, x2, dy, weight_shape, family='bf16x1'):
    """Weight gradient [O, I, 3, 3] of the 3x3 stride-1 pad-1 conv of cat(x1, x2) with x and dy rounded once to bf16
    (ssg_conv2d_wgrad_bf16x1_f32), or, family 'bf16x2', split into two bf16 terms (ssg_conv2d_wgrad_bf16x2_f32).  Returns None, with nothing launched, where ssg_conv2d_wgrad_bf16x1_ok refuses: the caller
    then takes _conv_wgrad_impl for this launch."""
    o, i, kh, kw = weight_shape
    if (kh, kw) != (3, 3) or tuple(dy.shape[2:]) != tuple(x1.shape[2:]) or x1.shape[1] + (x2.shape[1] if x2 is not None else 0) != i:
        return None
    d = _wgrad_desc(x1, x1.shape[1], x2, x2.shape[1] if x2 is not None else 0, dy, weight_shape, 1, _X1_TAPS)
    if not call('ssg_conv2d_wgrad_%s_ok' % family, C.byref(d)):
        return None
    n, _, h, w = x1.shape
    dw = torch.empty((o, i, 3, 3), device=dy.device, dtype=torch.float32)
    d.dw_oihw = dw.data_ptr()
    ws = _ws(call('ssg_conv2d_wgrad_%s_workspace_bytes' % family, C.byref(d)), dy.device)
    d.ws = ws.data_ptr(); d.ws_bytes = ws.numel() * 8
    _timed_call(_WGRAD_X2_KIND if family == 'bf16x2' else _WGRAD_X1_KIND, 'ssg_conv2d_wgrad_%s_f32' % family, d, (), (n, h, w, i, o, 3, 1),
                2.0 * n * h * w * o * i * 9)
    return dw


# csrc/conv_wgrad_s2_k32_x1.hip: the stride-2 form, behind a switch of its own (wgrad_s2).  Labels in a table of their own.
_WGRAD_X1_S2_LABELS = {81: 'wgrad_s2_k32_x1_kernel<128>', 82: 'wgrad_s2_k32_x1_kernel<64>'}
_WGRAD_X1_S2_KIND = (_WGRAD_X1_S2_LABELS, 'ssg_conv2d_wgrad_bf16x1_s2_kernel_id', _WGRAD_SHAPE)


def _conv_wgrad_s2_bf16x1_impl(x, dy, weight_shape):
    """Weight gradient [O, I, 3, 3] of the 3x3 stride-2 pad-1 conv of x with x and dy rounded once to bf16
    (ssg_conv2d_wgrad_bf16x1_s2_f32).  Returns None, with nothing launched, where ssg_conv2d_wgrad_bf16x1_s2_ok refuses: the
    caller then takes _conv_wgrad_impl's fp32-class kernel for this launch."""
    o, i, kh, kw = weight_shape
    n, c, h, w = x.shape
    if (kh, kw) != (3, 3) or c != i or tuple(dy.shape) != (n, o, (h + 1) // 2, (w + 1) // 2):
        return None
    d = _wgrad_desc(x, c, None, 0, dy, weight_shape, 2, _X1_TAPS)
    if not call('ssg_conv2d_wgrad_bf16x1_s2_ok', C.byref(d)):
        return None
    oh, ow = dy.shape[2], dy.shape[3]
    dw = torch.empty((o, i, 3, 3), device=dy.device, dtype=torch.float32)
    d.dw_oihw = dw.data_ptr()
    ws = _ws(call('ssg_conv2d_wgrad_bf16x1_s2_workspace_bytes', C.byref(d)), dy.device)
    d.ws = ws.data_ptr(); d.ws_bytes = ws.numel() * 8
    _timed_call(_WGRAD_X1_S2_KIND, 'ssg_conv2d_wgrad_bf16x1_s2_f32', d, (), (n, oh, ow, i, o, 3, 2), 2.0 * n * oh * ow * o * i * 9)
    return dw


def _conv_dgrad_bf16x1_impl(dy, weight, h, w, c_lo, c_hi, res=None, family='bf16x1'):
    """Input gradient of the 3x3 stride-1 pad-1 conv for input channels [c_lo, c_hi) with dy and the weight rounded once to bf16:
    conv_halo_k32_x1_kernel on dy with rows [c_lo, c_hi) of the transposed kmode-0 pack and the taps (1 - ky, 1 - kx); `res` is
    added in the epilogue (family 'bf16x2': conv_halo_k32_x2_kernel, two terms).  Returns None, with nothing launched, where ssg_conv2d_bf16x1_ok refuses (the caller then takes
    _conv_dgrad_impl for this launch)."""
    o, i, kh, kw = weight.shape
    n, _, oh, ow = dy.shape
    rows = c_hi - c_lo
    if (kh, kw) != (3, 3) or (oh, ow) != (h, w) or o % 16 or rows <= 0:
        return None
    d = _x1_desc(dy, None, weight, res)
    d.Cout = rows; d.ldo = pad4(rows); d.Kp = 9 * o
    _fill_taps(d, _X1_TAPS_T)
    if not call('ssg_conv2d_%s_ok' % family, C.byref(d)):
        return None
    wpk, kp, kmode = _pack(weight, 1, _X1_TAPS_T, o, o)
    dx = new_nhwc(n, rows, h, w, dy.device)
    d.w = wpk.data_ptr() + c_lo * kp * 4; d.Kp = kp; d.kmode = kmode
    d.out = dx.data_ptr(); d.ldo = _ld(dx)
    fmt = call('ssg_conv2d_%s_ok' % family, C.byref(d))
    if not fmt:
        return None
    pack = _x1_pack(weight, wpk, kp, fmt, transpose=1, row0=c_lo, rows=rows, family=family)
    _timed_call(_x_kind(family), 'ssg_conv2d_%s_f32' % family, d, (ptr(pack),), (n, h, w, o, rows, 9, 1, 1), 2.0 * n * h * w * o * rows * 9)
    return dx


# ----------------------------------------------------------------------------- opt-in bf16x1: the stride-2 conv of the single-conv node
# csrc/conv_s2_k32_x1.hip: the 3x3 stride-2 pad-1 forward (ssg_conv2d_bf16x1_s2_f32) and its input gradient as four parity-class
# launches (ssg_conv2d_bf16x1_cls_f32; the tap lists are those of the per-class launches of _conv_dgrad_impl).  Reached only from
# _Conv2d under precision='bf16x1'; the stride-2 weight gradient stays on the fp32-class kernel unless wgrad_s2='bf16x1' asks for
# _conv_wgrad_s2_bf16x1_impl above.  Labels in tables of their own.
_X1_S2_LABELS = {73: 'conv_s2_k32_x1_kernel<128,9>', 74: 'conv_s2_k32_x1_kernel<64,9>'}
_X1_CLS_LABELS = {75: 'conv_s2_k32_x1_kernel<128,1>', 76: 'conv_s2_k32_x1_kernel<64,1>', 77: 'conv_s2_k32_x1_kernel<128,2>',
                  78: 'conv_s2_k32_x1_kernel<64,2>', 79: 'conv_s2_k32_x1_kernel<128,4>', 80: 'conv_s2_k32_x1_kernel<64,4>'}
_X1_S2_KIND = (_X1_S2_LABELS, 'ssg_conv2d_bf16x1_s2_kernel_id', _CONV_SHAPE)
_X1_CLS_KIND = (_X1_CLS_LABELS, 'ssg_conv2d_bf16x1_cls_kernel_id', _CONV_SHAPE)


def _s2_classes():
    """(py, px, taps) of the four output-parity classes of a 3x3 stride-2 pad-1 input gradient: _conv_dgrad_impl's lists."""
    return [(py, px, [(ky, kx, (py + 1 - ky) // 2, (px + 1 - kx) // 2) for ky in range(3) for kx in range(3)
                      if (py + 1 - ky) % 2 == 0 and (px + 1 - kx) % 2 == 0]) for py in range(2) for px in range(2)]


def _x1_s2_desc(x, weight, out=None):
    """ssg_conv_desc of the stride-2 bf16x1 forward for these tensors (stand-in pointers as in _x1_desc)."""
    ld = nhwc_ld(x)
    n, c1, h, w = x.shape
    o = weight.shape[0]
    oh, ow = _out_hw(h, w, 3, 3, 2, 1)
    return _conv_desc((x.data_ptr(), ld) if ld is not None else (16, pad4(c1)), c1, None, 0, (n, h, w), 16, 9 * c1, 0, None, None,
                      _at(out) if out is not None else (16, pad4(o)), o, (oh, ow, oh, ow), 2, 1, (0, 0), _X1_TAPS, ACT_NONE, 0.0)


def conv2d_bf16x1_s2_ok(x, weight):
    """True where the stride-2 bf16x1 forward takes these tensors (ssg_conv2d_bf16x1_s2_ok): a 3x3 weight, Cin % 32 == 0,
    Cout % 64 == 0, an output at least 17 pixels wide, fp32 tensors below 4 GiB.  Launches nothing."""
    if not _x1_shapes_ok(x, weight, None, None) or min(x.shape[2:]) < 1:
        return False
    return call('ssg_conv2d_bf16x1_s2_ok', C.byref(_x1_s2_desc(x, weight))) != 0


def _conv_s2_bf16x1_impl(x, weight, bias, act, slope, out=None):
    """act(conv3x3(x, weight, stride 2, padding 1) + bias) with x and the weight rounded once to bf16.  Returns None, with nothing
    launched, where ssg_conv2d_bf16x1_s2_ok refuses (the caller then takes the fp32-class kernel)."""
    if not _x1_shapes_ok(x, weight, None, None):
        return None
    x = to_nhwc(x.detach())
    n, c1, h, w = x.shape
    o = weight.shape[0]
    d = _x1_s2_desc(x, weight, out)
    if not call('ssg_conv2d_bf16x1_s2_ok', C.byref(d)):
        return None
    wpk, kp, kmode = _pack(weight, 0, _X1_TAPS, c1, c1)
    oh, ow = _out_hw(h, w, 3, 3, 2, 1)
    if out is None:
        out = new_nhwc(n, o, oh, ow, x.device)
    d.out, d.ldo = _at(out)
    d.w = wpk.data_ptr(); d.Kp = kp; d.kmode = kmode
    d.bias = bias.data_ptr() if bias is not None else None
    d.act = int(act); d.slope = float(slope)
    fmt = call('ssg_conv2d_bf16x1_s2_ok', C.byref(d))
    if not fmt:
        return None
    pack = _x1_pack(weight, wpk, kp, fmt)
    _timed_call(_X1_S2_KIND, 'ssg_conv2d_bf16x1_s2_f32', d, (ptr(pack),), (n, oh, ow, c1, o, 9, 2, 1), 2.0 * n * oh * ow * o * c1 * 9, tag=_ROLE[0])
    return out


def _x1_cls_pack(weight, wpk, kp, taps, fmt, row0, rows):
    """The bf16 pack of rows [row0, row0 + rows) of the transposed kmode-0 matrix `wpk` for one parity class's taps
    (ssg_pack_weights_bf16x1_taps), cached beside the other bf16x1 packs of the weight."""
    cache = _stamped_cache(weight, '_ssg_pack_bf16x1')
    key = ('cls', tuple(taps), row0, rows, fmt)
    hit = cache.get(key)
    if hit is None:
        nbytes = call('ssg_pack_weights_bf16x1_taps_bytes', rows, kp, len(taps), fmt)
        hit = torch.empty(nbytes // 2, dtype=torch.int16, device=weight.device)
        call('ssg_pack_weights_bf16x1_taps', wpk.data_ptr() + row0 * kp * 4, rows, kp, len(taps), fmt, ptr(hit), stream_ptr())
        cache[key] = hit
    return hit


def _conv_dgrad_s2_bf16x1_impl(dy, weight, h, w, c_lo, c_hi, out=None):
    """Input gradient [N, c_hi - c_lo, h, w] of the 3x3 stride-2 pad-1 conv with dy and the weight rounded once to bf16: four
    launches of ssg_conv2d_bf16x1_cls_f32, one per output-parity class, each written at stride 2 and offset (py, px).  Returns None,
    with nothing launched or allocated, unless ssg_conv2d_bf16x1_cls_ok takes all four classes."""
    o, i, kh, kw = weight.shape
    n, _, oh, ow = dy.shape
    rows = c_hi - c_lo
    if (kh, kw) != (3, 3) or (oh, ow) != _out_hw(h, w, 3, 3, 2, 1) or o % 16 or rows <= 0 or dy.dtype != torch.float32 or weight.dtype != torch.float32:
        return None
    dy = to_nhwc(dy.detach())
    descs = []
    for py, px, taps in _s2_classes():
        gh, gw = (h - py + 1) // 2, (w - px + 1) // 2
        d = _conv_desc(_at(dy), o, None, 0, (n, oh, ow), 16, len(taps) * o, 0, None, None, _at(out) if out is not None else (16, pad4(rows)), rows,
                       (gh, gw, h, w), 1, 2, (py, px), taps, ACT_NONE, 0.0)
        if not call('ssg_conv2d_bf16x1_cls_ok', C.byref(d)):
            return None
        descs.append((d, taps, gh, gw))
    dx = out if out is not None else new_nhwc(n, rows, h, w, dy.device)
    for d, taps, gh, gw in descs:
        wpk, kp, kmode = _pack(weight, 1, taps, o, o)
        d.w = wpk.data_ptr() + c_lo * kp * 4; d.Kp = kp; d.kmode = kmode
        d.out, d.ldo = _at(dx)
        fmt = call('ssg_conv2d_bf16x1_cls_ok', C.byref(d))
        if not fmt:
            raise RuntimeError('conv bf16x1 cls: the predicate changed its answer between the check and the launch')
        pack = _x1_cls_pack(weight, wpk, kp, taps, fmt, c_lo, rows)
        _timed_call(_X1_CLS_KIND, 'ssg_conv2d_bf16x1_cls_f32', d, (ptr(pack),), (n, gh, gw, o, rows, len(taps), 1, 2), 2.0 * n * gh * gw * o * rows * len(taps))
    return dx


def conv2d_bf16x1_train(x, weight, bias=None, act=ACT_NONE, slope=0.0, x2=None, res=None, stride=1, wgrad_s2='fp32'):
    """The differentiable form of `conv2d_bf16x1`: forward on conv_halo_k32_x1_kernel, gradients for x, x2 and res on the same
    kernel (dy and the transposed weight rounded to bf16), weight gradient on wgrad_k32_x1_kernel (x and dy rounded), bias gradient
    by the fp32 channel sum.  A gradient whose own predicate refuses (a 32-channel slice, say) runs on the fp32-class kernel.
    stride=2 (no x2 / res): forward and input gradient on conv_s2_k32_x1_kernel where `conv2d_bf16x1_s2_ok` holds, the weight
    gradient on the fp32-class kernel, or with wgrad_s2='bf16x1' on wgrad_s2_k32_x1_kernel where its predicate holds.  Raises
    ValueError where `conv2d_bf16x1_ok` / `conv2d_bf16x1_s2_ok` is false or wgrad_s2 is neither 'fp32' nor 'bf16x1'; there is no
    CPU fallback."""
    _lib.require_gpu(x)
    weight = param('conv2d_bf16x1_train', 'weight', weight, x, packed=True)
    bias = param('conv2d_bf16x1_train', 'bias', bias, x)
    for t in (x2, res):
        if t is not None:
            _lib.require_gpu(t)
    _check_wgrad_s2('conv2d_bf16x1_train', 'bf16x1', wgrad_s2)
    if stride == 2:
        if x2 is not None or res is not None or not conv2d_bf16x1_s2_ok(x, weight):
            raise ValueError('conv2d_bf16x1_train: no stride-2 bf16x1 kernel for x %s weight %s%s (conv2d_bf16x1_s2_ok is False)' % (
                tuple(x.shape), tuple(weight.shape), ' with x2 / res' if (x2 is not None or res is not None) else ''))
        return _Conv2d.apply(x, None, weight, bias, 2, 1, int(act), float(slope), None, False, 'bf16x1', wgrad_s2)[0]
    if stride != 1:
        raise ValueError('conv2d_bf16x1_train: stride %r (1 or 2)' % (stride,))
    if not conv2d_bf16x1_ok(x, weight, x2=x2, res=res):
        raise ValueError('conv2d_bf16x1_train: no bf16x1 kernel for x %s x2 %s weight %s res %s (conv2d_bf16x1_ok is False)' % (
            tuple(x.shape), None if x2 is None else tuple(x2.shape), tuple(weight.shape), None if res is None else tuple(res.shape)))
    return _Conv2d.apply(x, x2, weight, bias, 1, 1, int(act), float(slope), res, False, 'bf16x1')[0]


# ----------------------------------------------------------------------------- linear (as 1x1 conv over a 1 x N "image")
class _Linear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, act, slope):
        n, k = x.shape
        o = weight.shape[0]
        if k % 4 or x.stride(1) != 1 or x.stride(0) % 4 or x.data_ptr() % 16:
            x = _pad_rows(x)
        xi = x.as_strided((1, k, 1, n), (n * x.stride(0), 1, n * x.stride(0), x.stride(0)))
        if weight.is_contiguous() and weight.data_ptr() % 16 == 0 and k % 4 == 0:
            # skinny GEMM that streams the [O][K] parameter once (HBM-bound); no packed copy
            y = new_nhwc(1, o, 1, n, x.device)
            nbytes = call('ssg_linear_fwd_workspace_bytes', n, k, o)
            ws = _ws(nbytes, x.device)
            call('ssg_linear_fwd_f32', ptr(xi), n, k, x.stride(0), ptr(weight), o, ptr(bias) if bias is not None else None,
                 act, slope, ptr(y), _ld(y), ptr(ws), nbytes, stream_ptr())
        else:
            y = _conv_fwd_impl(xi, None, weight.view(o, k, 1, 1), bias, 1, 0, act, slope)      # [1, o, 1, n]
        ld = _ld(y)
        y2 = torch.empty(0, device=y.device, dtype=torch.float32).set_(y.untyped_storage(), y.storage_offset(), (n, o), (ld, 1))
        ctx.save_for_backward(xi, weight, y if act != ACT_NONE else None)
        ctx.cfg = (act, slope, n, k, o, bias is not None)
        return y2

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy2):
        xi, weight, y = ctx.saved_tensors
        act, slope, n, k, o, has_bias = ctx.cfg
        if dy2.stride(1) != 1 or dy2.stride(0) % 4 or dy2.stride(0) < pad4(o) or dy2.data_ptr() % 16 or (o % 4 and dy2.stride(0) != pad4(o)):
            dy2 = _pad_rows(dy2)
        ldd = dy2.stride(0)
        dy = dy2.as_strided((1, o, 1, n), (n * ldd, 1, n * ldd, ldd))
        if act != ACT_NONE:
            dy = _act_bwd(y, dy, act, slope)
        w4 = weight.view(o, k, 1, 1)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            d = _conv_dgrad_impl(dy, w4, 1, 0, 1, n, 0, k)
            dx = d.as_strided((n, k), (_ld(d), 1))
        if ctx.needs_input_grad[1]:
            if k % 4 == 0 and xi.data_ptr() % 16 == 0 and xi.stride(3) % 4 == 0:
                dw = torch.empty((o, k), device=dy.device, dtype=torch.float32)
                call('ssg_linear_wgrad_f32', ptr(xi), n, k, xi.stride(3), ptr(dy), o, dy.stride(3), ptr(dw), stream_ptr())
            else:
                dw = _conv_wgrad_impl(xi, None, dy, (o, k, 1, 1), 1, 0).view(o, k)
        if has_bias and ctx.needs_input_grad[2]:
            db = _channel_sum(dy, o)
        return dx, dw, db, None, None


def _pad_rows(x):
    """Copy a [n, k] matrix into a zero-padded [n, pad4(k)] buffer (tiny tensors only)."""
    n, k = x.shape
    buf = torch.zeros((n, pad4(k)), device=x.device, dtype=torch.float32)
    xi = x.detach().contiguous().view(n, k, 1, 1)
    call('ssg_nchw_to_nhwc_f32', ptr(xi), n, k, 1, 1, ptr(buf), pad4(k), stream_ptr())
    return buf[:, :k]


def linear(x, weight, bias=None, act=ACT_NONE, slope=0.0):
    _lib.require_gpu(x)
    # (a strided weight is copied here, not at pack time: the skinny GEMM streams the parameter itself and keeps no pack)
    return _Linear.apply(x, param('linear', 'weight', weight, x), param('linear', 'bias', bias, x), int(act), float(slope))


# ----------------------------------------------------------------------------- batch norm (+residual, +activation)
def _synced(group):
    """True when batch-norm sums have to travel: a process group is attached and the job is distributed
    (world > 1, or SSG_DIST_FORCE=1 -- dp.FORCE -- which sends a single rank's collectives through the backend too)."""
    if group is None or not (dist.is_available() and dist.is_initialized()):
        return False
    from . import dp
    return dist.get_world_size(group) > 1 or dp.FORCE


# bumped whenever a training-mode batch norm rewrites running statistics through raw pointers (tensor version counters do
# not see that): part of the stamp of every eval-mode BN-fold cache (archs.BasicBlock._folded)
_STATS_EPOCH = [0]


BN_FUSED_FINALIZE = _os.environ.get('SSG_BN_FUSED_FINALIZE', '1') != '0'

# SSG_BN_BWD_LEAN (like blocks.SPADE_BWD_LEAN): 0 = the sequence before DESIGN.md 3.25 -- a batch norm with a residual keeps its fp32
# output for the backward's activation mask, and a conv bias gradient in front of a batch norm / behind an activation is a
# ssg_channel_sum_f32 pass over the freshly written gradient; 1 = the lean one: the forward packs the mask into C / 8 bytes per pixel
# (ssg_bn_apply_mask_f32) where ssg_bn_mask_ok allows it, ConvolutionalBlock's conv -> BN -> act is one node whose apply pass carries
# sum(dx) (ssg_bn_bwd_apply_sums_f32), and a conv's activation backward and bias gradient are one ssg_bn_frozen_bwd_f32 sweep;
# 2 = the same without the size threshold (tests).  Every lean form computes the bits of the sequence it replaces.
# BN_BWD_LEAN_MIN (elements of the tensor) holds for the mask forms alone: they keep the launch count, so below a size the C / 8
# extra bytes per pixel of the forward are all that changes.  Trace of the 16 x 512^2 step (profiles/r16_a_*): the residual layers
# of 3.1 M and 8.4 M elements come out within +-3 us of the old sequence over their three launches, the 25 M one gains 34 us --
# the threshold sits between them.  The other two forms drop a launch and a pass at every size and have no threshold.
BN_BWD_LEAN = {'0': 0, '2': 2}.get(_os.environ.get('SSG_BN_BWD_LEAN', '1'), 1)
BN_BWD_LEAN_MIN = 1 << 24


def _bn_lean(numel=None):
    """The lean switch; with `numel`, for a form that BN_BWD_LEAN_MIN governs."""
    return BN_BWD_LEAN == 2 or (BN_BWD_LEAN == 1 and (numel is None or numel >= BN_BWD_LEAN_MIN))


def _bn_mask_route(x, res, act):
    """True where the forward of a batch norm saves the 1-bit mask instead of its output: a residual (without one the mask is
    recomputed from x), fp32, and what ssg_bn_mask_ok asks of (C, act)."""
    return bool(res is not None and x.dtype == torch.float32 and _bn_lean(x.numel()) and call('ssg_bn_mask_ok', x.shape[1], act))


def bn_fin(weight, bias, eps, momentum, var_mode, running_mean, running_var, stats):
    """ctypes `ssg_bn_fin` over the given tensors (stats = [mean, invstd, scale, shift] rows)."""
    f = _lib.BnFin()
    f.weight = weight.data_ptr() if weight is not None else None
    f.bias = bias.data_ptr() if bias is not None else None
    f.eps = eps; f.momentum = momentum; f.var_mode = var_mode
    f.running_mean = running_mean.data_ptr() if running_mean is not None else None
    f.running_var = running_var.data_ptr() if running_var is not None else None
    f.mean = stats[0].data_ptr(); f.invstd = stats[1].data_ptr(); f.scale = stats[2].data_ptr(); f.shift = stats[3].data_ptr()
    return f


def _bn_fwd_impl(x, weight, bias, running_mean, running_var, res, eps, momentum, act, slope, var_mode, group, part=None, apply=True,
                 want_mask=False):
    """Timed wrapper (bench.py `hbm_stages`): algorithmic bytes per SURVEY.md 8(d) -- 2 reads + 1 write of the tensor, one read
    less when the statistics rode the producing conv's epilogue, one more for a residual (and the mask bytes where they are
    written).  `want_mask`: returns (y, stats, count, mask) -- see _bn_fwd_body."""
    n, c, h, w = x.shape
    reads = (1 if (part is not None and part.numel() > 0) else 2) + (1 if res is not None else 0)
    if not apply:                 # statistics only (the consumer conv applies scale / shift / act on its input): no pass over x at all
        reads -= 1
    masked = want_mask and apply and _bn_mask_route(x, res, act)
    with _hbm('bn_fwd', 4.0 * n * h * w * c * (reads + (1 if apply else 0)) + (n * h * w * c / 8.0 if masked else 0.0)):
        r = _bn_fwd_body(x, weight, bias, running_mean, running_var, res, eps, momentum, act, slope, var_mode, group, part, apply, masked)
    return (r if masked else r + (None,)) if want_mask else r


def _bn_apply(x, stats, res, act, slope):
    """y = act(x * scale + shift (+ res)) with the finalized statistics rows [mean, invstd, scale, shift]."""
    n, c, h, w = x.shape
    y = new_nhwc(n, c, h, w, x.device)
    call('ssg_bn_apply_f32', ptr(x), n * h * w, c, _ld(x), ptr(stats[2]), ptr(stats[3]), ptr(res), _ld(res) if res is not None else 0,
         act, slope, ptr(y), _ld(y), stream_ptr())
    return y


def _bn_apply_mask(x, stats, res, act, slope):
    """_bn_apply that also packs the sign of what it stores (ssg_bn_apply_mask_f32): returns (y, mask) -- the same y, and uint8
    [pixels, C / 8] with bit c % 8 of byte c / 8 = y > 0."""
    n, c, h, w = x.shape
    y = new_nhwc(n, c, h, w, x.device)
    mask = torch.empty((n * h * w, c // 8), dtype=torch.uint8, device=x.device)
    call('ssg_bn_apply_mask_f32', ptr(x), n * h * w, c, _ld(x), ptr(stats[2]), ptr(stats[3]), ptr(res), _ld(res) if res is not None else 0,
         act, slope, ptr(y), _ld(y), ptr(mask), c // 8, stream_ptr())
    return y, mask


def _bn_fwd_body(x, weight, bias, running_mean, running_var, res, eps, momentum, act, slope, var_mode, group, part=None, apply=True,
                 masked=False):
    """stats -> (all-reduce) -> finalize -> apply.  Returns (y, stats[4,C], count): `count` is None for a local batch norm
    and, when synchronised, the fp64[1] device tensor holding the all-reduced pixel count (ranks may hold unequal batches:
    the count travels with the sums instead of being assumed to be p * world).  `masked`: the apply also packs the 1-bit
    activation mask (_bn_apply_mask), returned as a fourth."""
    n, c, h, w = x.shape
    if c % 4:
        raise ValueError('batch_norm: C %% 4 != 0 unsupported (C=%d)' % c)
    p = n * h * w
    dev = x.device
    synced = _synced(group)
    stats = torch.empty((4, c), dtype=torch.float32, device=dev)      # mean, invstd, scale, shift
    have_part = part is not None and part.numel() > 0
    if have_part and (part.shape[-1] != c or part.numel() % (2 * c)):
        raise ValueError('batch_norm: statistics partials %s do not fit C=%d' % (tuple(part.shape), c))
    if not synced and BN_FUSED_FINALIZE:
        # local batch norm: the second reduce stage finishes the channel (one launch less; same bits as stats + finalize)
        fin = bn_fin(weight, bias, eps, momentum, var_mode, running_mean, running_var, stats)
        if have_part:
            rows = part.numel() // (2 * c)
            ws = _ws(call('ssg_bn_stats_from_partials_workspace_bytes', rows, c), dev)
            call('ssg_bn_stats_from_partials_finalize_f32', ptr(part), rows, c, float(p), C.byref(fin), ptr(ws), stream_ptr())
        else:
            ws = _ws(call('ssg_bn_workspace_bytes', p, c), dev)
            call('ssg_bn_stats_finalize_f32', ptr(x), p, c, _ld(x), C.byref(fin), ptr(ws), stream_ptr())
        sums = None
    else:
        sums = torch.empty(2 * c + 1, dtype=torch.float64, device=dev)
        if have_part:
            # (sum x, sum x^2) came out of the producing conv's epilogue, one row per tile: x is not read for its statistics
            rows = part.numel() // (2 * c)
            ws = _ws(call('ssg_bn_stats_from_partials_workspace_bytes', rows, c), dev)
            call('ssg_bn_stats_from_partials_f32', ptr(part), rows, c, ptr(sums), float(p) if synced else 0.0, ptr(ws), stream_ptr())
        else:
            ws = _ws(call('ssg_bn_workspace_bytes', p, c), dev)
            call('ssg_bn_stats_f32', ptr(x), p, c, _ld(x), ptr(sums), int(synced), ptr(ws), stream_ptr())
        if synced:
            _timed_all_reduce('sync_bn_fwd', sums, group)
        call('ssg_bn_finalize_f32', ptr(sums), 0.0 if synced else float(p), c, ptr(weight), ptr(bias), eps, momentum, var_mode,
             ptr(running_mean), ptr(running_var), ptr(stats[0]), ptr(stats[1]), ptr(stats[2]), ptr(stats[3]), stream_ptr())
    if running_mean is not None or running_var is not None:
        _STATS_EPOCH[0] += 1
    cnt = sums[2 * c:] if synced else None
    if apply and masked:
        y, mask = _bn_apply_mask(x, stats, res, act, slope)
        return y, stats, cnt, mask
    y = _bn_apply(x, stats, res, act, slope) if apply else None
    return y, stats, cnt


def _bn_bwd_impl(x, y, dy, weight, stats, act, slope, group, count, want_dres, want_dx=True, had_res=True, mask=None, want_dxsum=False):
    """Timed wrapper (bench.py `hbm_stages`): algorithmic bytes per SURVEY.md 8(d) -- 3 reads + 1 write (x, dy, the mask source;
    dx), plus the dres write where the forward had a residual.  With the 1-bit `mask` the mask source is C / 8 bytes per pixel
    instead of a tensor."""
    n, c, h, w = x.shape
    src = n * h * w * c / 8.0 if mask is not None else 4.0 * n * h * w * c
    with _hbm('bn_bwd', 4.0 * n * h * w * c * (2 + (1 if want_dx else 0) + (1 if want_dres else 0)) + src):
        return _bn_bwd_body(x, y, dy, weight, stats, act, slope, group, count, want_dres, want_dx, had_res, mask, want_dxsum)


def _bn_bwd_body(x, y, dy, weight, stats, act, slope, group, count, want_dres, want_dx=True, had_res=True, mask=None, want_dxsum=False):
    """Returns (dx, dres, dweight, dbias), and sum(dx) per channel as a fifth where `want_dxsum` (the apply pass carries it:
    ssg_bn_bwd_apply_sums_f32, the bits of _channel_sum(dx)).  The activation mask is read from the 1-bit `mask` the forward
    packed, else from y, or -- when the forward had no residual (`had_res=False`) -- recomputed from x with the forward's
    (scale, shift): y is then not read.  `count`: what _bn_fwd_impl returned (None = local batch norm)."""
    n, c, h, w = x.shape
    p = n * h * w
    dev = x.device
    if act == ACT_NONE or not had_res:
        y = mask = None
    if mask is not None:
        y = None
    synced = count is not None
    ws = _ws(call('ssg_bn_workspace_bytes', p, c), dev)
    sums = torch.empty(2 * c + 1, dtype=torch.float64, device=dev)
    if mask is not None:
        call('ssg_bn_bwd_reduce_mask_f32', ptr(x), ptr(mask), ptr(dy), p, c, _ld(x), mask.shape[1], _ld(dy),
             ptr(stats[0]), ptr(stats[1]), act, slope, ptr(sums), int(synced), ptr(ws), stream_ptr())
    else:
        call('ssg_bn_bwd_reduce_f32', ptr(x), ptr(y), ptr(dy), p, c, _ld(x), _ld(y) if y is not None else 0, _ld(dy),
             ptr(stats[0]), ptr(stats[1]), ptr(stats[2]), ptr(stats[3]), act, slope, ptr(sums), int(synced), ptr(ws), stream_ptr())
    # local (un-reduced) sums are this rank's weight/bias gradients; data-parallel all-reduces them later
    local = sums.clone() if synced else sums
    if synced:
        _timed_all_reduce('sync_bn_bwd', sums, group)
    dwb = torch.empty((2, c), dtype=torch.float32, device=dev)
    dx = new_nhwc(n, c, h, w, dev) if want_dx else None
    dres = new_nhwc(n, c, h, w, dev) if want_dres else None
    dxsum = None
    if want_dxsum:
        dxsum = torch.empty(c, dtype=torch.float32, device=dev)
        call('ssg_bn_bwd_apply_sums_f32', ptr(x), ptr(y), ptr(mask), ptr(dy), p, c, _ld(x), _ld(y) if y is not None else 0,
             mask.shape[1] if mask is not None else 0, _ld(dy), ptr(stats[0]), ptr(stats[1]), ptr(weight), ptr(stats[2]), ptr(stats[3]),
             ptr(sums), 0.0 if synced else float(p), act, slope, ptr(dx), _ld(dx), ptr(dres), _ld(dres) if dres is not None else 0,
             ptr(dwb[0]), ptr(dwb[1]), ptr(dxsum), ptr(ws), stream_ptr())
    elif mask is not None:
        call('ssg_bn_bwd_apply_mask_f32', ptr(x), ptr(mask), ptr(dy), p, c, _ld(x), mask.shape[1], _ld(dy),
             ptr(stats[0]), ptr(stats[1]), ptr(weight), ptr(sums), 0.0 if synced else float(p), act, slope,
             ptr(dx), _ld(dx) if dx is not None else 0, ptr(dres), _ld(dres) if dres is not None else 0,
             ptr(dwb[0]), ptr(dwb[1]), stream_ptr())
    else:
        call('ssg_bn_bwd_apply_f32', ptr(x), ptr(y), ptr(dy), p, c, _ld(x), _ld(y) if y is not None else 0, _ld(dy),
             ptr(stats[0]), ptr(stats[1]), ptr(weight), ptr(stats[2]), ptr(stats[3]), ptr(sums), 0.0 if synced else float(p), act, slope,
             ptr(dx), _ld(dx) if dx is not None else 0, ptr(dres), _ld(dres) if dres is not None else 0,
             ptr(dwb[0]), ptr(dwb[1]), stream_ptr())
    if synced:
        dwb = torch.stack([local[c:2 * c], local[:c]]).float()
    return (dx, dres, dwb[0], dwb[1], dxsum) if want_dxsum else (dx, dres, dwb[0], dwb[1])


# SSG_BN_BWD_EPILOGUE=1: bn1's backward sums of a residual block from the epilogue of conv2's input gradient (ssg_conv_desc.bwd_x) instead of
# a reduce pass over (dy1, c1).  Measured (same box, twice on two boxes): bn_bwd 14.4 -> 12.7 ms per step, and the k32 launches that carry
# the epilogue give it back (<8,128> -1.4 %, <16,64> -3 % over all their launches): 191.9 / 191.8 vs 192.1 / 191.9 ms, 189.6 / 190.9 vs
# 189.9 / 190.5.  Off by default.
BN_BWD_EPILOGUE = _os.environ.get('SSG_BN_BWD_EPILOGUE', '0') == '1'


def _bn_bwd_from_partials(x, g, part, weight, stats, group, count):
    """Batch-norm backward whose two sums came out of the producing input-gradient launch (ssg_conv_desc.bwd_x): g is already masked, `part`
    holds per-tile rows (sum g, sum g * (x - mean)).  Fold, scale the second sum by invstd (-> sum g * xhat), all-reduce when synchronised,
    apply.  Returns (dx, dweight, dbias) like _bn_bwd_impl."""
    n, c, h, w = x.shape
    p = n * h * w
    dev = x.device
    synced = count is not None
    rows = part.numel() // (2 * c)
    sums = torch.empty(2 * c + 1, dtype=torch.float64, device=dev)
    ws = _ws(call('ssg_bn_stats_from_partials_workspace_bytes', rows, c), dev)
    call('ssg_bn_stats_from_partials_f32', ptr(part), rows, c, ptr(sums), float(p) if synced else 0.0, ptr(ws), stream_ptr())
    sums[c:2 * c] *= stats[1].double()
    local = sums.clone() if synced else sums
    if synced:
        _timed_all_reduce('sync_bn_bwd', sums, group)
    dwb = torch.empty((2, c), dtype=torch.float32, device=dev)
    dx = new_nhwc(n, c, h, w, dev)
    with _hbm('bn_bwd', 4.0 * p * c * 3):
        call('ssg_bn_bwd_apply_f32', ptr(x), None, ptr(g), p, c, _ld(x), 0, _ld(g),
             ptr(stats[0]), ptr(stats[1]), ptr(weight), ptr(stats[2]), ptr(stats[3]), ptr(sums), 0.0 if synced else float(p), ACT_NONE, 0.0,
             ptr(dx), _ld(dx), None, 0, ptr(dwb[0]), ptr(dwb[1]), stream_ptr())
    if synced:
        dwb = torch.stack([local[c:2 * c], local[:c]]).float()
    return dx, dwb[0], dwb[1]


def _relabel(t, c):
    """The same NHWC-with-stride memory seen with `c` logical channels (c <= pixel stride); a base tensor, not a view."""
    n, _, h, w = t.shape
    return torch.empty(0, device=t.device, dtype=t.dtype).set_(t.untyped_storage(), t.storage_offset(), (n, c, h, w), t.stride())


class _BatchNormAct(torch.autograd.Function):
    """Channel counts that are not multiples of 4 (the 1-channel psi BatchNorm of Attention_block, archs.py:128-132)
    run on the padded lanes too: zero data with zero weight/bias stays zero."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, res, eps, momentum, act, slope, var_mode, group, part=None):
        x = to_nhwc(x)
        res = to_nhwc(res) if res is not None else None
        c = x.shape[1]
        c4 = pad4(c)
        if c4 != c:
            x = _relabel(x, c4)
            res = _relabel(res, c4) if res is not None else None
            wp = torch.nn.functional.pad(weight.detach(), (0, c4 - c)); bp = torch.nn.functional.pad(bias.detach(), (0, c4 - c))
            rm = torch.nn.functional.pad(running_mean, (0, c4 - c)) if running_mean is not None else None
            rv = torch.nn.functional.pad(running_var, (0, c4 - c), value=1.0) if running_var is not None else None
            y, stats, cnt = _bn_fwd_impl(x, wp, bp, rm, rv, res, eps, momentum, act, slope, var_mode, group)
            mask = None
            if running_mean is not None:
                running_mean.copy_(rm[:c])
            if running_var is not None:
                running_var.copy_(rv[:c])
            weight = wp
        else:
            y, stats, cnt, mask = _bn_fwd_impl(x, weight, bias, running_mean, running_var, res, eps, momentum, act, slope, var_mode, group,
                                               part=part, want_mask=True)
        # no residual: mask is recomputed; with one, the packed mask where the forward wrote it, else y
        ctx.save_for_backward(x, y if (act != ACT_NONE and res is not None and mask is None) else None, weight, stats, mask)
        ctx.cfg = (act, slope, group, cnt, res is not None, c)
        return _relabel(y, c) if c4 != c else y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, y, weight, stats, mask = ctx.saved_tensors
        act, slope, group, cnt, has_res, c = ctx.cfg
        dy = to_nhwc(dy)
        c4 = x.shape[1]
        if c4 != c:
            dy = _relabel(dy, c4)
        dx, dres, dw, db = _bn_bwd_impl(x, y, dy, weight, stats, act, slope, group, cnt, has_res and ctx.needs_input_grad[5],
                                        had_res=has_res, mask=mask)
        if c4 != c:
            dx = _relabel(dx, c)
            dres = _relabel(dres, c) if dres is not None else None
            dw, db = dw[:c].clone(), db[:c].clone()
        return dx, dw, db, None, None, dres, None, None, None, None, None, None, None


def _frozen_bwd(x, y, dy, mean, invstd, scale, shift, act, slope, want_dx=True, want_dres=False):
    """One sweep of ssg_bn_frozen_bwd_f32 over dy: (dx, dres, sums) with g = dy * act'(.), dx = g * scale (scale None: g),
    dres = g, sums = fp64 [sum g | sum g * xhat] (second half zero without mean).  x / y / mean / scale may be None as the
    entry point allows; the mask comes from y where it is given."""
    n, c, h, w = dy.shape
    p = n * h * w
    dev = dy.device
    dx = new_nhwc(n, c, h, w, dev) if want_dx else None
    dres = new_nhwc(n, c, h, w, dev) if want_dres else None
    sums = torch.empty(2 * c, dtype=torch.float64, device=dev)
    ws = _ws(call('ssg_bn_workspace_bytes', p, c), dev)
    reads = 1 + (x is not None) + (y is not None and act in (ACT_RELU, ACT_LRELU))
    with _hbm('bn_frozen_bwd', 4.0 * p * c * (reads + (1 if want_dx else 0) + (1 if want_dres else 0))):
        call('ssg_bn_frozen_bwd_f32', ptr(x), ptr(y), ptr(dy), p, c, _ld(x) if x is not None else 0, _ld(y) if y is not None else 0, _ld(dy),
             ptr(mean), ptr(invstd), ptr(scale), ptr(shift), act, slope, ptr(dx), _ld(dx) if dx is not None else 0,
             ptr(dres), _ld(dres) if dres is not None else 0, ptr(sums), ptr(ws), stream_ptr())
    return dx, dres, sums


class _AffineAct(torch.autograd.Function):
    """Eval-mode BN: y = x*scale + shift (+res) -> act with constant scale/shift (mean, invstd, scale, shift of the running
    estimates, already padded to the lanes the kernels run).  Differentiable in x, res, weight and bias: with constant
    statistics the backward is one pass (ssg_bn_frozen_bwd_f32), dweight = sum g*xhat, dbias = sum g."""

    @staticmethod
    def forward(ctx, x, weight, bias, mean, invstd, scale, shift, res, act, slope, record):
        x = to_nhwc(x)
        res = to_nhwc(res) if res is not None else None
        c = x.shape[1]
        c4 = scale.numel()
        if c4 != c:                                         # 1-channel psi batch norm: run the padded lanes with scale = shift = 0
            x = _relabel(x, c4)
            res = _relabel(res, c4) if res is not None else None
        n, _, h, w = x.shape
        y = new_nhwc(n, c4, h, w, x.device)
        call('ssg_bn_apply_f32', ptr(x), n * h * w, c4, _ld(x), ptr(scale), ptr(shift), ptr(res), _ld(res) if res is not None else 0,
             act, slope, ptr(y), _ld(y), stream_ptr())
        if record and any(ctx.needs_input_grad):          # `record`: the caller's grad mode (it is always off inside forward)
            # the rule of _BatchNormAct: y only with an activation AND a residual, otherwise the mask is recomputed from x;
            # x itself only where the backward reads it (recomputed mask, swish, or the weight gradient's xhat)
            keep_y = act in (ACT_RELU, ACT_LRELU) and res is not None
            keep_x = ctx.needs_input_grad[1] or (act != ACT_NONE and not keep_y)
            ctx.save_for_backward(x if keep_x else None, y if keep_y else None, mean, invstd, scale, shift)
            ctx.cfg = (act, slope, c)
        return _relabel(y, c) if c4 != c else y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, y, mean, invstd, scale, shift = ctx.saved_tensors
        act, slope, c = ctx.cfg
        dy = to_nhwc(dy)
        c4 = scale.numel()
        if c4 != c:
            dy = _relabel(dy, c4)
        need_x, need_w, need_b, need_res = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2], ctx.needs_input_grad[7]
        want_dres = bool(need_res)
        # identity case of the residual gradient: no activation -> dres = dy itself, nothing to write
        plain = act == ACT_NONE
        dx, dres, sums = _frozen_bwd(x, y, dy, mean if need_w else None, invstd if need_w else None, scale, shift, act, slope,
                                     want_dx=bool(need_x), want_dres=want_dres and not plain)
        if want_dres and plain:
            dres = dy
        if c4 != c:
            dx = _relabel(dx, c) if dx is not None else None
            dres = _relabel(dres, c) if dres is not None else None
        dw = sums[c4:c4 + c].float() if need_w else None
        db = sums[:c].float() if need_b else None
        return dx, dw, db, None, None, None, None, dres, None, None, None


def batch_norm_act(x, bn, res=None, act=ACT_NONE, slope=0.0, group=None, var_mode=None, stats_part=None):
    """nn.BatchNorm2d `bn` (any _BatchNorm holding weight/bias/running stats) + residual + activation.
    `stats_part`: the per-tile statistics the producing conv2d(..., bn_stats=True) returned (train mode only).
    A `bn` in eval mode (frozen: batchnorm.freeze_batch_norm) normalises with its running estimates, writes none of them, issues
    no collective and is differentiable in x, res, bn.weight and bn.bias."""
    _lib.require_gpu(x)
    bn_w, bn_b, bn_rm, bn_rv = bn_params('batch_norm_act', bn, x, stats=bn.track_running_stats)
    if bn.training or not bn.track_running_stats:
        if bn.momentum is None:
            raise NotImplementedError('cumulative-average batch norm (momentum=None)')
        if bn.track_running_stats and bn.num_batches_tracked is not None and not _synced(group):
            bn.num_batches_tracked.add_(1)           # the reference's synchronised branch never counts batches (batchnorm.py:57-80)
        if var_mode is None:
            var_mode = getattr(bn, '_ssg_var_mode', 1 if group is not None else 0)
        return _BatchNormAct.apply(x, bn_w, bn_b, bn_rm, bn_rv, res, float(bn.eps), float(bn.momentum),
                                   int(act), float(slope), int(var_mode), group, stats_part)
    with torch.no_grad():
        invstd = torch.rsqrt(bn_rv + bn.eps)
        scale = invstd
        if bn_w is not None:
            scale = scale * bn_w
        shift = -bn_rm * scale
        if bn_b is not None:
            shift = shift + bn_b
        c = scale.numel()
        mean = bn_rm
        if c % 4:                                           # 1-channel psi batch norm: the padded lanes run with scale = shift = 0
            scale = torch.nn.functional.pad(scale, (0, pad4(c) - c)); shift = torch.nn.functional.pad(shift, (0, pad4(c) - c))
    if c % 4 and torch.is_grad_enabled():                   # only a recorded forward needs the statistics on the padded lanes too
        with torch.no_grad():
            mean = torch.nn.functional.pad(mean, (0, pad4(c) - c)); invstd = torch.nn.functional.pad(invstd, (0, pad4(c) - c))
    record = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, res, bn_w, bn_b))
    if record and act == ACT_SWISH and res is not None:
        # (the kernel refuses the combination in any forward; said here by name where a graph would be recorded)
        raise NotImplementedError('batch_norm_act: swish with a residual has no backward (its derivative needs the pre-activation sum)')
    return _AffineAct.apply(x, bn_w, bn_b, mean, invstd, scale.contiguous(), shift.contiguous(), res, int(act), float(slope), record)


class _ConvBnAct(torch.autograd.Function):
    """conv (+bias) -> training-mode batch norm -> activation as ONE node (models_seg_gan.ConvolutionalBlock).  The forward is
    the launches of conv2d(bn_stats=True) + batch_norm_act; in the backward the conv's bias gradient sum(dx of the batch norm)
    comes out of the apply pass that writes dx (ssg_bn_bwd_apply_sums_f32) -- inside one node, so it travels in a local
    variable -- instead of a _channel_sum pass over the fresh tensor.  Same kernels otherwise, same bits."""

    @staticmethod
    def forward(ctx, x, weight, bias, bn_w, bn_b, running_mean, running_var, stride, pad, eps, momentum, act, slope, var_mode, group,
                precision, wgrad_s2):
        x = to_nhwc(x)
        c, part = _conv_fwd_impl(x, None, weight, bias, stride, pad, ACT_NONE, 0.0, want_bn=True, precision=precision, x1_s2=True)
        y, stats, cnt = _bn_fwd_impl(c, bn_w, bn_b, running_mean, running_var, None, eps, momentum, act, slope, var_mode, group, part=part)
        ctx.save_for_backward(x, weight, c, bn_w, stats)
        ctx.cfg = (stride, pad, act, slope, group, cnt, precision, wgrad_s2, bias is not None)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, weight, c, bn_w, stats = ctx.saved_tensors
        stride, pad, act, slope, group, cnt, precision, wgrad_s2, has_bias = ctx.cfg
        dy = to_nhwc(dy)
        need = ctx.needs_input_grad
        want_db = bool(has_bias and need[2])
        r = _bn_bwd_impl(c, None, dy, bn_w, stats, act, slope, group, cnt, want_dres=False, had_res=False, want_dxsum=want_db)
        dc, dg, dbeta, db = r[0], r[2], r[3], (r[4] if want_db else None)
        n, c1, h, w = x.shape
        dx = _conv_dgrad_impl(dc, weight, stride, pad, h, w, 0, c1, precision=precision, x1_s2=True) if need[0] else None
        dw = _conv_wgrad_impl(x, None, dc, weight.shape, stride, pad, precision=precision, wgrad_s2=wgrad_s2) if need[1] else None
        return (dx, dw, db, dg, dbeta) + (None,) * 12


def conv_bn_act_ok(x, weight, bn):
    """Whether conv_bn_act takes this layer: the lean switch, a batch norm in training mode, fp32, and an output channel count
    the batch-norm kernels run unpadded."""
    return bool(_bn_lean() and bn.training and bn.momentum is not None and
                x.dtype == torch.float32 and weight.shape[0] % 4 == 0)


def conv_bn_act(x, weight, bias, stride, padding, bn, act=ACT_NONE, slope=0.0, group=None, precision='fp32', wgrad_s2='fp32'):
    """batch_norm_act(conv2d(x, weight, bias, bn_stats=True), bn, act) as one autograd node (_ConvBnAct); the caller has asked
    conv_bn_act_ok.  Parameter contract, counters and precision arguments as in conv2d and batch_norm_act."""
    _lib.require_gpu(x)
    if precision not in _PRECISIONS:
        raise ValueError('conv_bn_act: unknown precision %r (one of %s)' % (precision, ', '.join(_PRECISIONS)))
    _check_wgrad_s2('conv_bn_act', precision, wgrad_s2)
    weight = param('conv2d', 'weight', weight, x, packed=True)
    bias = param('conv2d', 'bias', bias, x)
    bn_w, bn_b, bn_rm, bn_rv = bn_params('batch_norm_act', bn, x, stats=bn.track_running_stats)
    if bn.track_running_stats and bn.num_batches_tracked is not None and not _synced(group):
        bn.num_batches_tracked.add_(1)
    var_mode = getattr(bn, '_ssg_var_mode', 1 if group is not None else 0)
    pad = tuple(int(v) for v in padding) if isinstance(padding, (tuple, list)) else int(padding)
    return _ConvBnAct.apply(x, weight, bias, bn_w, bn_b, bn_rm, bn_rv, int(stride), pad, float(bn.eps), float(bn.momentum),
                            int(act), float(slope), int(var_mode), group, precision, wgrad_s2)


# ----------------------------------------------------------------------------- pool / unpool / upsample
class _MaxPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = to_nhwc(x)
        n, c, h, w = x.shape
        if c % 4 or h % 2 or w % 2:
            raise ValueError('max_pool2x2: needs C %% 4 == 0 and even H, W (got %s)' % (tuple(x.shape),))
        oh, ow = h // 2, w // 2
        y = new_nhwc(n, c, oh, ow, x.device)
        idx = torch.empty((n, oh, ow, c), dtype=torch.uint8, device=x.device)
        with _hbm('maxpool_fwd', n * h * w * c * (4.0 + 1.0 + 0.25)):        # 1 read + 1/4 write + 1/4 byte index per input element
            call('ssg_maxpool2x2_fwd_f32', ptr(x), n, h, w, c, _ld(x), ptr(y), _ld(y), ptr(idx), stream_ptr())
        ctx.save_for_backward(idx)
        ctx.hw = (h, w)
        ctx.mark_non_differentiable(idx)
        return y, idx

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy, _):
        (idx,) = ctx.saved_tensors
        dy = to_nhwc(dy)
        n, c, oh, ow = dy.shape
        h, w = ctx.hw
        dx = new_nhwc(n, c, h, w, dy.device)
        with _hbm('maxpool_bwd', n * h * w * c * (1.0 + 0.25 + 4.0)):
            call('ssg_maxpool2x2_bwd_f32', ptr(dy), _ld(dy), ptr(idx), n, h, w, c, ptr(dx), _ld(dx), stream_ptr())
        return dx


def max_pool2x2(x):
    """nn.MaxPool2d(2, 2, return_indices=True): returns (y, idx) with idx the 1-byte window argmax."""
    _lib.require_gpu(x)
    return _MaxPool.apply(x)


class _MaxPoolSkip(torch.autograd.Function):
    """max_pool2x2 of a tensor that ALSO feeds a skip connection: returns (y, idx, x_skip) with x_skip = x.  One autograd node
    receives both gradients and forms dx = d_skip + pool_backward(dy) in the pool-backward pass, so autograd never launches
    its own 3-tensor add for the encoder outputs (archs.py:628-667: up to 1 GB each at 16 x 512^2)."""

    @staticmethod
    def forward(ctx, x):
        x = to_nhwc(x)
        n, c, h, w = x.shape
        if c % 4 or h % 2 or w % 2:
            raise ValueError('max_pool2x2: needs C %% 4 == 0 and even H, W (got %s)' % (tuple(x.shape),))
        oh, ow = h // 2, w // 2
        y = new_nhwc(n, c, oh, ow, x.device)
        idx = torch.empty((n, oh, ow, c), dtype=torch.uint8, device=x.device)
        with _hbm('maxpool_fwd', n * h * w * c * (4.0 + 1.0 + 0.25)):        # 1 read + 1/4 write + 1/4 byte index per input element
            call('ssg_maxpool2x2_fwd_f32', ptr(x), n, h, w, c, _ld(x), ptr(y), _ld(y), ptr(idx), stream_ptr())
        ctx.save_for_backward(idx)
        ctx.hw = (h, w)
        ctx.mark_non_differentiable(idx)
        ctx.set_materialize_grads(False)       # an unused output arrives as None in backward, not as a zero tensor to scatter / add
        return y, idx, x

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy, _, dskip):
        (idx,) = ctx.saved_tensors
        h, w = ctx.hw
        if dy is None:
            return dskip
        dy = to_nhwc(dy)
        n, c, oh, ow = dy.shape
        dx = new_nhwc(n, c, h, w, dy.device)
        if dskip is None:
            with _hbm('maxpool_bwd', n * h * w * c * (1.0 + 0.25 + 4.0)):
                call('ssg_maxpool2x2_bwd_f32', ptr(dy), _ld(dy), ptr(idx), n, h, w, c, ptr(dx), _ld(dx), stream_ptr())
        else:
            dskip = to_nhwc(dskip)
            with _hbm('maxpool_bwd', n * h * w * c * (1.0 + 0.25 + 4.0 + 4.0)):      # + the skip gradient it adds
                call('ssg_maxpool2x2_bwd_add_f32', ptr(dy), _ld(dy), ptr(idx), ptr(dskip), _ld(dskip), n, h, w, c, ptr(dx), _ld(dx), stream_ptr())
        return dx


def max_pool2x2_skip(x):
    """(y, idx, x_skip): max_pool2x2(x) plus x handed back for a skip connection; use x_skip (not x) downstream."""
    _lib.require_gpu(x)
    return _MaxPoolSkip.apply(x)


class _MaxUnpool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, idx):
        x = to_nhwc(x)
        n, c, h, w = x.shape
        if tuple(idx.shape) != (n, h, w, c) or idx.dtype != torch.uint8:
            raise ValueError('max_unpool2x2: indices %s do not match input %s' % (tuple(idx.shape), tuple(x.shape)))
        y = new_nhwc(n, c, 2 * h, 2 * w, x.device)
        with _hbm('unpool_fwd', n * h * w * c * (4.0 + 1.0 + 16.0)):         # 1/4 read + 1/4 byte index + 1 write per output element
            call('ssg_maxunpool2x2_fwd_f32', ptr(x), _ld(x), ptr(idx), n, 2 * h, 2 * w, c, ptr(y), _ld(y), stream_ptr())
        ctx.save_for_backward(idx)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        (idx,) = ctx.saved_tensors
        dy = to_nhwc(dy)
        n, c, oh, ow = dy.shape
        dx = new_nhwc(n, c, oh // 2, ow // 2, dy.device)
        with _hbm('unpool_bwd', n * (oh // 2) * (ow // 2) * c * (4.0 + 1.0 + 4.0)):
            call('ssg_maxunpool2x2_bwd_f32', ptr(dy), _ld(dy), ptr(idx), n, oh, ow, c, ptr(dx), _ld(dx), stream_ptr())
        return dx, None


def max_unpool2x2(x, idx):
    _lib.require_gpu(x)
    return _MaxUnpool.apply(x, idx)


def _make_upsample(fwd_name, bwd_name, stage):
    class _Up(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            x = to_nhwc(x)
            n, c, h, w = x.shape
            if c % 4:
                raise ValueError('upsample2x: C %% 4 != 0')
            y = new_nhwc(n, c, 2 * h, 2 * w, x.device)
            with _hbm(stage + '_fwd', n * h * w * c * (4.0 + 16.0)):             # 1/4 read + 1 write per output element
                call(fwd_name, ptr(x), n, h, w, c, _ld(x), ptr(y), _ld(y), stream_ptr())
            return y

        @staticmethod
        @torch.autograd.function.once_differentiable
        def backward(ctx, dy):
            dy = to_nhwc(dy)
            n, c, oh, ow = dy.shape
            dx = new_nhwc(n, c, oh // 2, ow // 2, dy.device)
            with _hbm(stage + '_bwd', n * (oh // 2) * (ow // 2) * c * (16.0 + 4.0)):
                call(bwd_name, ptr(dy), _ld(dy), n, oh // 2, ow // 2, c, ptr(dx), _ld(dx), stream_ptr())
            return dx
    return _Up


_BilinearUp = _make_upsample('ssg_upsample2x_bilinear_fwd_f32', 'ssg_upsample2x_bilinear_bwd_f32', 'bilinear')
_NearestUp = _make_upsample('ssg_upsample2x_nearest_fwd_f32', 'ssg_upsample2x_nearest_bwd_f32', 'nearest')


def upsample2x_bilinear(x):
    """nn.Upsample(scale_factor=2, mode='bilinear', align_corners=True)."""
    _lib.require_gpu(x)
    return _BilinearUp.apply(x)


def upsample2x_nearest(x):
    """nn.Upsample(scale_factor=2) (nearest)."""
    _lib.require_gpu(x)
    return _NearestUp.apply(x)


class _AvgPoolFlat(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, o):
        x = to_nhwc(x)
        n, c, h, w = x.shape
        y = torch.empty((n, c * o * o), dtype=torch.float32, device=x.device)
        call('ssg_adaptive_avgpool_flat_fwd_f32', ptr(x), n, h, w, c, _ld(x), o, ptr(y), stream_ptr())
        ctx.cfg = (n, c, h, w, o)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        n, c, h, w, o = ctx.cfg
        dy = dy.contiguous()
        dx = new_nhwc(n, c, h, w, dy.device, zero=(c % 4 != 0))
        call('ssg_adaptive_avgpool_flat_bwd_f32', ptr(dy), n, h, w, c, o, ptr(dx), _ld(dx), stream_ptr())
        return dx, None


def adaptive_avgpool_flat(x, o=6):
    """nn.AdaptiveAvgPool2d((o, o)) followed by .view(N, -1) in NCHW order."""
    _lib.require_gpu(x)
    return _AvgPoolFlat.apply(x, int(o))


# ----------------------------------------------------------------------------- SPADE modulate
class _SpadeModulate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gb):
        x = to_nhwc(x); gb = to_nhwc(gb)
        n, c, h, w = x.shape
        if c % 4 or gb.shape[1] != 2 * c:
            raise ValueError('spade_modulate: x has %d channels, gamma|beta has %d' % (c, gb.shape[1]))
        y = new_nhwc(n, c, h, w, x.device)
        with _hbm('spade_modulate_fwd', 16.0 * n * h * w * c):                   # x, gamma, beta in; out
            call('ssg_spade_modulate_fwd_f32', ptr(x), _ld(x), ptr(gb), _ld(gb), n * h * w, c, ptr(y), _ld(y), stream_ptr())
        ctx.save_for_backward(x, gb)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, gb = ctx.saved_tensors
        dy = to_nhwc(dy)
        n, c, h, w = x.shape
        dx = new_nhwc(n, c, h, w, x.device)
        dgb = new_nhwc(n, 2 * c, h, w, x.device)
        call('ssg_spade_modulate_bwd_f32', ptr(x), _ld(x), ptr(gb), _ld(gb), ptr(dy), _ld(dy), n * h * w, c,
             ptr(dx), _ld(dx), ptr(dgb), _ld(dgb), stream_ptr())
        return dx, dgb


def spade_modulate(x, gb):
    """out = x*(1+gamma)+beta with gamma = gb[:, :C], beta = gb[:, C:] (normalization.py:120)."""
    _lib.require_gpu(x)
    return _SpadeModulate.apply(x, gb)


# ----------------------------------------------------------------------------- losses
class _SegLoss(torch.autograd.Function):
    """Fused BCEDiceLoss + MSELoss + IoU/Dice metrics.  Returns a float32[8] tensor `res`
    (layout in include/ssunet_hip.h); gradients flow from res[0] (BCEDice), res[1] (MSE) and res[2] (StableBCE);
    res[3:] are metrics (their incoming gradient is ignored, as the reference computes them in numpy)."""

    @staticmethod
    def forward(ctx, x, t, mc0):
        x = to_nhwc(x); t = to_nhwc(t)
        n, c, h, w = x.shape
        s = h * w
        dev = x.device
        res = torch.empty(8, dtype=torch.float32, device=dev)
        stats = torch.empty(3 * n + 5, dtype=torch.float64, device=dev)
        ws = _ws(call('ssg_seg_loss_workspace_bytes', n, s, c), dev)
        call('ssg_seg_loss_fwd_f32', ptr(x), _ld(x), ptr(t), _ld(t), n, s, c, mc0, ptr(res), ptr(stats), ptr(ws), stream_ptr())
        ctx.save_for_backward(x, t, res, stats)
        ctx.mark_non_differentiable(stats)
        return res, stats

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, _):
        x, t, res, stats = ctx.saved_tensors
        n, c, h, w = x.shape
        g = g.contiguous()
        dx = new_nhwc(n, c, h, w, x.device)
        call('ssg_seg_loss_bwd_f32', ptr(x), _ld(x), ptr(t), _ld(t), n, h * w, c, ptr(res), ptr(stats),
             C.c_void_p(g.data_ptr()), C.c_void_p(g.data_ptr() + 4), C.c_void_p(g.data_ptr() + 8), ptr(dx), _ld(dx), stream_ptr())
        return dx, None, None


def seg_loss(logits, target, metric_first_channel=1, with_sums=False):
    """Fused loss/metric pass.  Returns res (float32[8]); with_sums=True also returns the fp64[5]
    metric partial sums (for cross-rank reduction of IoU/Dice)."""
    _lib.require_gpu(logits)
    res, stats = _SegLoss.apply(logits, target, int(metric_first_channel))
    if with_sums:
        return res, stats[-5:]
    return res


class _BCEConst(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, label):
        n = x.numel()
        if x.dim() != 2 or x.shape[1] != 1:
            raise ValueError('bce_with_logits_const expects [N, 1] logits')
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        call('ssg_bce_logits_const_fwd_f32', ptr(x), n, x.stride(0), label, ptr(loss), stream_ptr())
        ctx.save_for_backward(x)
        ctx.label = label
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        n = x.shape[0]
        buf = torch.empty((n, 4), dtype=torch.float32, device=x.device)
        g = g.contiguous()
        call('ssg_bce_logits_const_bwd_f32', ptr(x), n, x.stride(0), ctx.label, ptr(g), ptr(buf), 4, stream_ptr())
        return buf[:, :1], None


def bce_with_logits_const(x, label):
    """nn.BCEWithLogitsLoss()(x, full_like(x, label)) for x of shape [N, 1]."""
    _lib.require_gpu(x)
    return _BCEConst.apply(x, float(label))


class _NanToZero(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ld = nhwc_ld(x) if x.dim() == 4 else None
        if ld is not None:                          # operate on the whole padded buffer
            n, c, h, w = x.shape
            if ld != pad4(c):                       # a channel slice of a wider buffer: the other lanes are somebody else's
                raise ValueError('nan_to_zero_: pixel stride %d is wider than the %d channels (channel slice of another tensor)' % (ld, c))
            dense = x.as_strided((n * h * w * ld,), (1,))
        elif x.is_contiguous():
            dense = x.view(-1)
        else:
            raise ValueError('nan_to_zero_: unsupported layout (stride %s)' % (x.stride(),))
        mask = torch.empty(dense.numel(), dtype=torch.uint8, device=x.device)
        call('ssg_nan_to_zero_f32', ptr(dense), dense.numel(), ptr(mask), stream_ptr())
        ctx.save_for_backward(mask)
        ctx.nhwc = ld is not None
        ctx.mark_dirty(x)
        return x

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        (mask,) = ctx.saved_tensors
        if ctx.nhwc:
            g = to_nhwc(g)
            n, c, h, w = g.shape
            ld = pad4(c)                            # the mask follows x's rows, and x was compact (forward)
            if _ld(g) != ld:                        # a channel slice of a wider gradient (concat / add hand such views up): its
                gc = new_nhwc(n, c, h, w, g.device)             # own lanes into compact rows first (c % 4 == 0 here, see nhwc_ld)
                call('ssg_copy_channels_f32', ptr(g), _ld(g), n * h * w, c, ptr(gc), ld, stream_ptr())
                g = gc
            out = new_nhwc(n, c, h, w, g.device)
            call('ssg_mask_zero_f32', ptr(g), ptr(mask), n * h * w * ld, ptr(out), stream_ptr())
            return out
        g = g.contiguous()
        out = torch.empty_like(g)
        call('ssg_mask_zero_f32', ptr(g), ptr(mask), g.numel(), ptr(out), stream_ptr())
        return out


def nan_to_zero_(x):
    """x[isnan(x)] = 0 in place, differentiable (train_seg_gan.py:190)."""
    _lib.require_gpu(x)
    return _NanToZero.apply(x)


# ----------------------------------------------------------------------------- depthwise conv (unwired rows A10/A11)
class _DwConv2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, stride, pad):
        x = to_nhwc(x)
        n, c, h, w = x.shape
        if c % 4 or weight.shape[0] != c or weight.shape[1] != 1:
            raise ValueError('dwconv2d: depthwise weight [C,1,KH,KW] with C %% 4 == 0 expected, got %s for C=%d' % (tuple(weight.shape), c))
        kh, kw = weight.shape[2:]
        pt, pb, pl, pr = _pad4(pad)
        oh, ow = _out_hw(h, w, kh, kw, stride, pad)
        y = new_nhwc(n, c, oh, ow, x.device)
        wc = weight.contiguous()
        call('ssg_dwconv2d_fwd_f32', ptr(x), n, h, w, c, _ld(x), ptr(wc), ptr(bias), kh, kw, stride, pt, pl, oh, ow, ptr(y), _ld(y), stream_ptr())
        ctx.save_for_backward(x, wc)
        ctx.cfg = (stride, pt, pl, oh, ow, bias is not None)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, wc = ctx.saved_tensors
        stride, pt, pl, oh, ow, has_bias = ctx.cfg
        dy = to_nhwc(dy)
        n, c, h, w = x.shape
        kh, kw = wc.shape[2:]
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = new_nhwc(n, c, h, w, x.device)
            call('ssg_dwconv2d_dgrad_f32', ptr(dy), _ld(dy), n, h, w, c, ptr(wc), kh, kw, stride, pt, pl, oh, ow, ptr(dx), _ld(dx), stream_ptr())
        if ctx.needs_input_grad[1]:
            dw = torch.empty_like(wc)
            ws = _ws(call('ssg_dwconv2d_wgrad_workspace_bytes', n, oh, ow, c, kh, kw), x.device)
            call('ssg_dwconv2d_wgrad_f32', ptr(x), n, h, w, c, _ld(x), ptr(dy), _ld(dy), kh, kw, stride, pt, pl, oh, ow, ptr(dw), ptr(ws), stream_ptr())
        if has_bias and ctx.needs_input_grad[2]:
            db = _channel_sum(dy, c)
        return dx, dw, db, None, None


def dwconv2d(x, weight, bias=None, stride=1, padding=0):
    """Depthwise F.conv2d (groups = C)."""
    _lib.require_gpu(x)
    weight = param('dwconv2d', 'weight', weight, x, packed=True)      # (the node reads weight.contiguous())
    bias = param('dwconv2d', 'bias', bias, x)
    pad = tuple(int(v) for v in padding) if isinstance(padding, (tuple, list)) else int(padding)
    return _DwConv2d.apply(x, weight, bias, int(stride), pad)


UNARY_SWISH, UNARY_SIGMOID, UNARY_GAUSSIAN = 0, 1, 2


class _Unary(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, op):
        x = to_nhwc(x)
        n, c, h, w = x.shape
        y = new_nhwc(n, c, h, w, x.device)
        call('ssg_unary_fwd_f32', ptr(x), _ld(x), n * h * w, c, op, ptr(y), _ld(y), stream_ptr())
        ctx.save_for_backward(x)
        ctx.op = op
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        dy = to_nhwc(dy)
        n, c, h, w = x.shape
        dx = new_nhwc(n, c, h, w, x.device)
        call('ssg_unary_bwd_f32', ptr(x), _ld(x), ptr(dy), _ld(dy), n * h * w, pad4(c), ctx.op, ptr(dx), _ld(dx), stream_ptr())
        return dx, None


def swish(x):
    """x * sigmoid(x) with the reference's hand-written backward (efficientnet_pytorch/utils.py:37-48)."""
    _lib.require_gpu(x)
    return _Unary.apply(x, UNARY_SWISH)


def sigmoid(x):
    _lib.require_gpu(x)
    return _Unary.apply(x, UNARY_SIGMOID)


def gaussian(x):
    """exp(-x*x) (xresidualblock.py:5-7)."""
    _lib.require_gpu(x)
    return _Unary.apply(x, UNARY_GAUSSIAN)


def sigmoid_into(x, out):
    """sigmoid(x) written into `out`, an NHWC tensor of x's shape (or a batch slice of one) -- inference only, no autograd:
    the launch of `sigmoid` with another destination."""
    _lib.require_gpu(x)
    _lib.require_gpu(out)
    x = to_nhwc(x.detach())
    if out.shape != x.shape:
        raise ValueError('sigmoid_into: out is %s, x is %s' % (tuple(out.shape), tuple(x.shape)))
    n, c, h, w = x.shape
    call('ssg_unary_fwd_f32', ptr(x), _ld(x), n * h * w, c, UNARY_SIGMOID, ptr(out), _ld(out), stream_ptr())
    return out


# ----------------------------------------------------------------------------- sliding-window inference (csrc/sliding_window.hip)
_SW_NORM = []


def _sw_norm_consts():
    """mean * 255 and 1 / (std * 255) of albumentations Normalize(): the numpy expressions of
    aerial_image_segmentation_api.normalize_imagenet, so that the kernel multiplies by the very same fp32 values."""
    if not _SW_NORM:
        import numpy as np
        mean = np.array((0.485, 0.456, 0.406), dtype=np.float32) * 255.0
        std = np.array((0.229, 0.224, 0.225), dtype=np.float32) * 255.0
        denom = np.reciprocal(std, dtype=np.float32)
        _SW_NORM.append([float(v) for v in mean] + [float(v) for v in denom])
    return _SW_NORM[0]


def _sw_origins(origins, device):
    """(host int32 [P, 2] tensor, its device copy) of a list of patch origins (h1, w1): the entry points check the host copy
    and the kernels read the device one."""
    host = torch.as_tensor(origins, dtype=torch.int32, device='cpu').contiguous()
    if host.dim() != 2 or host.shape[1] != 2 or host.shape[0] == 0:
        raise ValueError('origins: expected P >= 1 pairs (h1, w1), got shape %s' % (tuple(host.shape),))
    return host, host.to(device)


def _sw_factor(p_size, size, who):
    if size <= 0 or p_size not in (size, 2 * size):
        raise NotImplementedError('%s: patch %d at %d: only the exact factors 1 and 2 are built' % (who, p_size, size))


def _sw_inside(host, p_size, img_h, img_w, who):
    h1, w1 = host[:, 0], host[:, 1]
    if bool(((h1 < 0) | (w1 < 0) | (h1 > img_h - p_size) | (w1 > img_w - p_size)).any()):
        raise ValueError('%s: a patch of size %d lies outside the %d x %d image' % (who, p_size, img_h, img_w))


TTA_SETS = {'hflip': (0, 4), 'flips': (0, 4, 2, 6), 'd4': (0, 1, 2, 3, 4, 5, 6, 7)}


def tta_codes(tta):
    """The D4 codes of a test-time-augmentation request, as a tuple: `None` -> (0,); a name of TTA_SETS ('hflip': identity and
    left-right flip; 'flips': identity, left-right, 180 degrees, up-down; 'd4': all eight); or a tuple / list of 1, 2, 4 or 8
    distinct codes.  Code k stands for T_k(a) = rot90(fliplr(a) if k >> 2 else a, k & 3), rot90 counter-clockwise
    (DESIGN.md 3.23).  Anything else raises ValueError."""
    if tta is None:
        return (0,)
    if isinstance(tta, str):
        if tta not in TTA_SETS:
            raise ValueError('tta %r: expected None, one of %s, or a tuple of 1, 2, 4 or 8 distinct D4 codes' % (tta, sorted(TTA_SETS)))
        return TTA_SETS[tta]
    if not isinstance(tta, (tuple, list)):
        raise ValueError('tta %r: expected None, one of %s, or a tuple of 1, 2, 4 or 8 distinct D4 codes' % (tta, sorted(TTA_SETS)))
    codes = tuple(tta)
    if len(codes) not in (1, 2, 4, 8):
        raise ValueError('tta %r: %d views; the mean is a balanced tree over 1, 2, 4 or 8' % (tta, len(codes)))
    for k in codes:
        if isinstance(k, bool) or not isinstance(k, int) or not 0 <= k <= 7:
            raise ValueError('tta %r: %r is no D4 code (an int in 0 .. 7)' % (tta, k))
    if len(set(codes)) != len(codes):
        raise ValueError('tta %r: a code is repeated' % (tta,))
    return codes


def sw_gather_patches(img_u8, origins, p_size, out_size, orient=0):
    """Network input of the sliding-window pipeline from the image on the device: for every origin (h1, w1) the
    p_size x p_size crop of `img_u8` ([H, W, 3] uint8, BGR), resized to out_size (p_size / out_size in {1, 2}), normalised
    and divided by 255 exactly as `get_patched_input` does on the host.  Returns [P, 3, out_size, out_size] fp32 NHWC
    (ld 4, pad lane 0).  `origins`: P pairs (h1, w1).  `orient`: a D4 code (`tta_codes`); every patch comes out as T_orient of
    what orient = 0 gives, bit for bit, the symmetry folded into the kernel's index map.  0 is the call it has always been."""
    if isinstance(orient, bool) or not isinstance(orient, int) or not 0 <= orient <= 7:
        raise ValueError('sw_gather_patches: orient %r is no D4 code (an int in 0 .. 7)' % (orient,))
    _lib.require_gpu(img_u8)
    if img_u8.dtype != torch.uint8 or img_u8.dim() != 3 or img_u8.shape[2] != 3 or not img_u8.is_contiguous():
        raise TypeError('sw_gather_patches: expected a contiguous [H, W, 3] uint8 image, got %s %s' % (img_u8.dtype, tuple(img_u8.shape)))
    _sw_factor(p_size, out_size, 'sw_gather_patches')
    host, devo = _sw_origins(origins, img_u8.device)
    img_h, img_w = img_u8.shape[0], img_u8.shape[1]
    _sw_inside(host, p_size, img_h, img_w, 'sw_gather_patches')
    n = host.shape[0]
    out = new_nhwc(n, 3, out_size, out_size, img_u8.device)
    if orient == 0:
        call('ssg_sw_gather_patches_u8_f32', ptr(img_u8), img_h, img_w, ptr(devo), ptr(host), n, p_size, out_size,
             *(_sw_norm_consts() + [ptr(out), stream_ptr()]))
    else:
        call('ssg_sw_gather_patches_d4_u8_f32', ptr(img_u8), img_h, img_w, ptr(devo), ptr(host), n, p_size, out_size, orient,
             *(_sw_norm_consts() + [ptr(out), stream_ptr()]))
    return out


def new_tta_stack(k, n, c, s, device):
    """[k, n, c, s, s] fp32 over one [k, n, s, s, ld] buffer (ld = c rounded up to 4): stack[i] is an NHWC tensor like
    `new_nhwc(n, c, s, s)`, stack[:, :m] the first m samples of every view -- what `sw_tta_reduce` takes."""
    ld = pad4(c)
    buf = torch.empty(k * n * s * s * ld, device=device, dtype=torch.float32)
    return torch.empty(0, device=device, dtype=torch.float32).set_(
        buf.untyped_storage(), 0, (k, n, c, s, s), (n * s * s * ld, s * s * ld, 1, s * ld, ld))


def sw_tta_reduce(stack, codes, out=None):
    """The test-time-augmentation mean on the device: `stack` is [K, B, C, S, S] fp32, view k the NHWC probabilities
    `sigmoid(model(T_codes[k] x))` (a `new_tta_stack` tensor or a slice of one, or a list of K NHWC tensors of one shape at a
    constant distance inside one allocation); the result is the mean over k of T_codes[k]^-1(stack[k]) -- a balanced tree of fp32
    adds in list order times 1 / K, so K equal views give back that view bit for bit -- as [B, C, S, S] NHWC with zero pad lanes,
    written into `out` (such a tensor, or a batch slice of one) if given.  `codes`: K = 1, 2, 4 or 8 distinct D4 codes
    (`tta_codes`); anything else raises ValueError before any launch.  The pad lanes of the views are never read into a result."""
    codes = tta_codes(codes)
    if isinstance(stack, (tuple, list)):
        views = list(stack)
    else:
        if stack.dim() != 5:
            raise ValueError('sw_tta_reduce: expected a [K, B, C, S, S] stack, got %s' % (tuple(stack.shape),))
        views = [stack[i] for i in range(stack.shape[0])]
    if len(views) != len(codes):
        raise ValueError('sw_tta_reduce: %d views for %d codes' % (len(views), len(codes)))
    v0 = views[0]
    for v in views:
        _lib.require_gpu(v)
    if v0.dim() != 4 or v0.shape[2] != v0.shape[3]:
        raise ValueError('sw_tta_reduce: expected views of [B, C, S, S], got %s' % (tuple(v0.shape),))
    ld = _ld(v0)
    slab = (views[1].data_ptr() - v0.data_ptr()) // 4 if len(views) > 1 else 0
    for i, v in enumerate(views):
        if v.shape != v0.shape or v.device != v0.device or _ld(v) != ld or v.data_ptr() != v0.data_ptr() + 4 * slab * i:
            raise ValueError('sw_tta_reduce: the views must be NHWC tensors of one shape, one pixel stride and a constant distance')
    b, c, s, _ = v0.shape
    if len(views) > 1 and (slab < b * s * s * ld or slab % 4):
        raise ValueError('sw_tta_reduce: the views overlap (distance %d floats, %d each)' % (slab, b * s * s * ld))
    if out is None:
        out = new_nhwc(b, c, s, s, v0.device)
    else:
        _lib.require_gpu(out)
        if out.shape != v0.shape or out.device != v0.device:
            raise ValueError('sw_tta_reduce: out is %s, a view is %s' % (tuple(out.shape), tuple(v0.shape)))
    host_codes = (C.c_int32 * len(codes))(*codes)
    call('ssg_sw_tta_reduce_f32', ptr(v0), slab, ld, len(codes), host_codes, b, c, s, ptr(out), _ld(out), stream_ptr())
    return out


def sw_merge_masks(probs, origins, weights, p_size, img_h, img_w):
    """`patch_merge` on the device: probs [P, C, S, S] fp32 (NHWC, as `sigmoid(model(x))` leaves them; p_size / S in {1, 2}),
    one origin and one int weight (multiplicity) per patch -> [C, img_h, img_w] uint8 masks in {0, 255}."""
    _lib.require_gpu(probs)
    if probs.dim() != 4 or probs.shape[2] != probs.shape[3]:
        raise ValueError('sw_merge_masks: expected [P, C, S, S] probabilities, got %s' % (tuple(probs.shape),))
    probs = to_nhwc(probs.detach())
    n, c, s, _ = probs.shape
    _sw_factor(p_size, s, 'sw_merge_masks')
    host, devo = _sw_origins(origins, probs.device)
    wt = torch.as_tensor(weights, dtype=torch.int32, device='cpu').contiguous()
    if host.shape[0] != n or wt.shape != (n,) or bool((wt < 0).any()):
        raise ValueError('sw_merge_masks: %d patches need %d origins and %d non-negative weights' % (n, n, n))
    _sw_inside(host, p_size, img_h, img_w, 'sw_merge_masks')
    out = torch.empty((c, img_h, img_w), dtype=torch.uint8, device=probs.device)
    wdev = wt.to(probs.device)
    call('ssg_sw_merge_masks_f32_u8', ptr(probs), _ld(probs), n, c, s, ptr(devo), ptr(host), ptr(wdev),
         p_size, img_h, img_w, ptr(out), stream_ptr())
    return out


def sw_gather_labels(label_u8, origins, p_size, out_size, classes=3):
    """The ground-truth patches of the sliding-window pipeline from the label image on the device: for every origin (h1, w1)
    and class c < classes, `mask_convert(label[h1:h1 + p_size, w1:w1 + p_size], c, out_size) / 255.0` of the host path
    (p_size / out_size in {1, 2}).  `label_u8`: contiguous [H, W, 3] uint8, BGR.  Returns [P, classes, out_size, out_size]
    fp32 NHWC (ld 4, pad lanes 0) holding 0.0 or 1.0 -- what `sw_merge_masks` takes."""
    _lib.require_gpu(label_u8)
    if label_u8.dtype != torch.uint8 or label_u8.dim() != 3 or label_u8.shape[2] != 3 or not label_u8.is_contiguous():
        raise TypeError('sw_gather_labels: expected a contiguous [H, W, 3] uint8 label image, got %s %s' % (label_u8.dtype, tuple(label_u8.shape)))
    _sw_factor(p_size, out_size, 'sw_gather_labels')
    if not 1 <= classes <= 3:
        raise ValueError('sw_gather_labels: %r classes: the label palette (mask_convert) has 3 colours' % (classes,))
    host, devo = _sw_origins(origins, label_u8.device)
    img_h, img_w = label_u8.shape[0], label_u8.shape[1]
    _sw_inside(host, p_size, img_h, img_w, 'sw_gather_labels')
    n = host.shape[0]
    out = new_nhwc(n, classes, out_size, out_size, label_u8.device)
    call('ssg_sw_gather_labels_u8_f32', ptr(label_u8), img_h, img_w, ptr(devo), ptr(host), n, p_size, out_size, classes,
         ptr(out), stream_ptr())
    return out


def sw_mask_counts(pred, gt, out=None):
    """Per class, the pixel counts (pred > 127 and gt > 127, pred > 127, gt > 127) of two uint8 mask sets [C, H, W] (or [C, HW])
    on the device, as an int64 [C, 3] device tensor.  `out`: such a tensor to ADD the counts into (and return) -- an evaluation
    loop accumulates over images without a host round trip."""
    _lib.require_gpu(pred)
    _lib.require_gpu(gt)
    if pred.dtype != torch.uint8 or gt.dtype != torch.uint8 or pred.dim() < 2 or pred.shape != gt.shape:
        raise TypeError('sw_mask_counts: expected two uint8 [C, H, W] mask sets of one shape, got %s %s and %s %s'
                        % (pred.dtype, tuple(pred.shape), gt.dtype, tuple(gt.shape)))
    if not (pred.is_contiguous() and gt.is_contiguous()):
        raise TypeError('sw_mask_counts: the mask sets must be contiguous')
    c = pred.shape[0]
    hw = pred.numel() // c if c else 0
    if c == 0 or hw == 0:
        raise ValueError('sw_mask_counts: empty mask set %s' % (tuple(pred.shape),))
    if out is None:
        out = torch.zeros((c, 3), dtype=torch.int64, device=pred.device)
    else:
        _lib.require_gpu(out)
        if out.dtype != torch.int64 or tuple(out.shape) != (c, 3) or not out.is_contiguous() or out.device != pred.device:
            raise TypeError('sw_mask_counts: out must be a contiguous int64 [%d, 3] tensor on %s' % (c, pred.device))
    call('ssg_sw_mask_counts_u8', ptr(pred), ptr(gt), c, hw, ptr(out), stream_ptr())
    return out


def sw_levels(thresholds, classes, who='sw_merge_scores'):
    """The per-class first-stage levels of a `thresholds` request, as a list of `classes` ints: an int in 0 .. 254 stands for
    every class, a tuple / list gives one such int per class.  Bools and anything else raise ValueError."""
    def level(v):
        if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v <= 254:
            raise ValueError('%s: threshold %r is no level (an int in 0 .. 254)' % (who, v))
        return v
    if isinstance(thresholds, (tuple, list)):
        if len(thresholds) != classes:
            raise ValueError('%s: %d thresholds for %d classes' % (who, len(thresholds), classes))
        return [level(v) for v in thresholds]
    return [level(thresholds)] * classes


def sw_merge_scores(probs, origins, weights, p_size, img_h, img_w, thresholds=None):
    """The confidence map of `patch_merge` on the device (host oracle: `patch_merge_scores`): arguments as
    `sw_merge_masks`; returns [C, img_h, img_w] uint8 scores S -- the number of first-stage levels t in 0 .. 254 at which
    `patch_merge`, thresholding every patch at t instead of 127, turns the pixel on; `(S > 127) * 255` is `sw_merge_masks`.
    `thresholds`: an int level or one per class (`sw_levels`, at most 64 classes) -- then the {0, 255} masks `S[c] > level[c]`
    come back instead, from one walk over the patches."""
    _lib.require_gpu(probs)
    if probs.dim() != 4 or probs.shape[2] != probs.shape[3]:
        raise ValueError('sw_merge_scores: expected [P, C, S, S] probabilities, got %s' % (tuple(probs.shape),))
    probs = to_nhwc(probs.detach())
    n, c, s, _ = probs.shape
    _sw_factor(p_size, s, 'sw_merge_scores')
    levels = None
    if thresholds is not None:
        if c > 64:
            raise ValueError('sw_merge_scores: thresholds for %d classes: at most 64 classes take levels' % c)
        levels = (C.c_int32 * c)(*sw_levels(thresholds, c))
    host, devo = _sw_origins(origins, probs.device)
    wt = torch.as_tensor(weights, dtype=torch.int32, device='cpu').contiguous()
    if host.shape[0] != n or wt.shape != (n,) or bool((wt < 0).any()):
        raise ValueError('sw_merge_scores: %d patches need %d origins and %d non-negative weights' % (n, n, n))
    _sw_inside(host, p_size, img_h, img_w, 'sw_merge_scores')
    out = torch.empty((c, img_h, img_w), dtype=torch.uint8, device=probs.device)
    wdev = wt.to(probs.device)
    call('ssg_sw_merge_scores_f32_u8', ptr(probs), _ld(probs), n, c, s, ptr(devo), ptr(host), ptr(wdev),
         p_size, img_h, img_w, levels, ptr(out), stream_ptr())
    return out


def sw_score_hist(scores, gt, out=None):
    """Per class c and ground-truth bit g = (gt > 127), the 256-bin histogram of the score bytes: uint8 [C, H, W] (or [C, HW])
    score maps and ground-truth masks on the device -> int64 [C, 2, 256] device tensor, hist[c, g, s] pixels.  `out`: such a
    tensor to ADD into (and return), so that a loop accumulates over images without a host round trip.  The counts of
    `sw_mask_counts` at any level t are suffix sums: I = hist[c, 1, t + 1:].sum(), P = hist[c, :, t + 1:].sum(), G = hist[c, 1].sum()."""
    _lib.require_gpu(scores)
    _lib.require_gpu(gt)
    if scores.dtype != torch.uint8 or gt.dtype != torch.uint8 or scores.dim() < 2 or scores.shape != gt.shape:
        raise TypeError('sw_score_hist: expected uint8 [C, H, W] scores and masks of one shape, got %s %s and %s %s'
                        % (scores.dtype, tuple(scores.shape), gt.dtype, tuple(gt.shape)))
    if not (scores.is_contiguous() and gt.is_contiguous()):
        raise TypeError('sw_score_hist: the scores and the masks must be contiguous')
    c = scores.shape[0]
    hw = scores.numel() // c if c else 0
    if c == 0 or hw == 0:
        raise ValueError('sw_score_hist: empty score map %s' % (tuple(scores.shape),))
    if out is None:
        out = torch.zeros((c, 2, 256), dtype=torch.int64, device=scores.device)
    else:
        _lib.require_gpu(out)
        if out.dtype != torch.int64 or tuple(out.shape) != (c, 2, 256) or not out.is_contiguous() or out.device != scores.device:
            raise TypeError('sw_score_hist: out must be a contiguous int64 [%d, 2, 256] tensor on %s' % (c, scores.device))
    call('ssg_sw_score_hist_u8', ptr(scores), ptr(gt), c, hw, ptr(out), stream_ptr())
    return out


# ----------------------------------------------------------------------------- training augmentation (csrc/augment.hip)
AUG_ROW = 16             # int32 entries of a parameter row: m0 .. m5 (16.16), flags, dh, ds, dv, six zeros (augment.py builds them)


def augment_batch(img_u8, mask_u8, params, luts, out_h, out_w, border=(0, 0, 0), out=None):
    """Network input and target of a training batch from uint8 tiles on the device, in one launch:
    `img_u8` [N, H, W, 3] (B, G, R) and `mask_u8` [N, H, W, C] (C in 1 .. 8), contiguous uint8 on one HIP device; `params` the
    HOST int32 [N, 16] table and `luts` the HOST uint8 [N, 256] tables of `augment.sample_params` (numpy arrays or CPU tensors).
    Per sample: one affine resampling (bilinear image taps, `border` bytes outside the source; nearest masks, 0 outside), the
    integer HSV shift where the row's flag asks for it, the brightness / contrast table, Normalize.  Returns
    ([N, 3, out_h, out_w], [N, C, out_h, out_w]) fp32 NHWC with zero pad lanes -- `new_nhwc` tensors, which the generator and
    `seg_loss` take as they are; `out`: such a pair to write into.  tests/augment_ref.py is the definition, bit for bit.
    Anything else raises before a launch."""
    _lib.require_gpu(img_u8)
    _lib.require_gpu(mask_u8)
    if img_u8.dtype != torch.uint8 or img_u8.dim() != 4 or img_u8.shape[3] != 3 or not img_u8.is_contiguous():
        raise TypeError('augment_batch: expected contiguous [N, H, W, 3] uint8 images, got %s %s' % (img_u8.dtype, tuple(img_u8.shape)))
    if mask_u8.dtype != torch.uint8 or mask_u8.dim() != 4 or mask_u8.shape[:3] != img_u8.shape[:3] or not mask_u8.is_contiguous():
        raise TypeError('augment_batch: expected contiguous [N, H, W, C] uint8 masks beside %s images, got %s %s'
                        % (tuple(img_u8.shape), mask_u8.dtype, tuple(mask_u8.shape)))
    if mask_u8.device != img_u8.device:
        raise TypeError('augment_batch: images on %s, masks on %s' % (img_u8.device, mask_u8.device))
    n, h, w, c = mask_u8.shape
    if n == 0 or h == 0 or w == 0 or not 1 <= c <= 8:
        raise ValueError('augment_batch: %d samples of %d x %d with %d mask channels (1 .. 8 are built)' % (n, h, w, c))
    if out_h <= 0 or out_w <= 0:
        raise ValueError('augment_batch: output %d x %d' % (out_h, out_w))
    host = torch.as_tensor(params).contiguous()
    tabs = torch.as_tensor(luts).contiguous()
    if host.is_cuda or host.dtype != torch.int32 or tuple(host.shape) != (n, AUG_ROW):
        raise TypeError('augment_batch: params must be a host int32 [%d, %d] table, got %s %s' % (n, AUG_ROW, host.dtype, tuple(host.shape)))
    if tabs.is_cuda or tabs.dtype != torch.uint8 or tuple(tabs.shape) != (n, 256):
        raise TypeError('augment_batch: luts must be host uint8 [%d, 256] tables, got %s %s' % (n, tabs.dtype, tuple(tabs.shape)))
    border = tuple(int(b) for b in border)
    if len(border) != 3 or not all(0 <= b <= 255 for b in border):
        raise ValueError('augment_batch: border %r is no byte triple' % (border,))
    dev = img_u8.device
    if out is None:
        inp, tgt = new_nhwc(n, 3, out_h, out_w, dev), new_nhwc(n, c, out_h, out_w, dev)
    else:
        inp, tgt = out
        for t, ch in ((inp, 3), (tgt, c)):
            if tuple(t.shape) != (n, ch, out_h, out_w) or t.device != dev or nhwc_ld(t) != pad4(ch):
                raise TypeError('augment_batch: out must be new_nhwc(%d, %d, %d, %d) tensors on %s' % (n, ch, out_h, out_w, dev))
    dev_params, dev_tabs = host.to(dev), tabs.to(dev)          # named: both must outlive the launch's enqueue
    call('ssg_augment_batch_u8_f32', ptr(img_u8), ptr(mask_u8), n, h, w, c, ptr(dev_params), ptr(host), ptr(dev_tabs),
         out_h, out_w, *(list(border) + _sw_norm_consts() + [ptr(inp), ptr(tgt), stream_ptr()]))
    return inp, tgt


class _Mul(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        a = to_nhwc(a); b = to_nhwc(b)
        n, c, h, w = a.shape
        y = new_nhwc(n, c, h, w, a.device)
        call('ssg_mul_fwd_f32', ptr(a), _ld(a), ptr(b), _ld(b), n * h * w, pad4(c), ptr(y), _ld(y), stream_ptr())
        ctx.save_for_backward(a, b)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        a, b = ctx.saved_tensors
        dy = to_nhwc(dy)
        n, c, h, w = a.shape
        da = new_nhwc(n, c, h, w, a.device); db = new_nhwc(n, c, h, w, a.device)
        call('ssg_mul_bwd_f32', ptr(a), _ld(a), ptr(b), _ld(b), ptr(dy), _ld(dy), n * h * w, pad4(c),
             ptr(da), _ld(da), ptr(db), _ld(db), stream_ptr())
        return da, db


def mul(a, b):
    _lib.require_gpu(a)
    return _Mul.apply(a, b)


class _PixelGate(torch.autograd.Function):
    """x * sigmoid(g) with a one-channel gate g broadcast over the channels (Attention_block, archs.py:138-144)."""

    @staticmethod
    def forward(ctx, x, g):
        x = to_nhwc(x); g = to_nhwc(g)
        n, c, h, w = x.shape
        if tuple(g.shape) != (n, 1, h, w):
            raise ValueError('pixel_gate: gate must be [N,1,H,W], got %s' % (tuple(g.shape),))
        y = new_nhwc(n, c, h, w, x.device)
        call('ssg_pixel_gate_fwd_f32', ptr(x), _ld(x), ptr(g), _ld(g), n * h * w, pad4(c), ptr(y), _ld(y), stream_ptr())
        ctx.save_for_backward(x, g)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, g = ctx.saved_tensors
        dy = to_nhwc(dy)
        n, c, h, w = x.shape
        dx = new_nhwc(n, c, h, w, x.device); dg = new_nhwc(n, 1, h, w, x.device)
        call('ssg_pixel_gate_bwd_f32', ptr(x), _ld(x), ptr(g), _ld(g), ptr(dy), _ld(dy), n * h * w, pad4(c),
             ptr(dx), _ld(dx), ptr(dg), _ld(dg), stream_ptr())
        return dx, dg


def pixel_gate(x, g):
    _lib.require_gpu(x)
    return _PixelGate.apply(x, g)


class _GlobalAvgPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = to_nhwc(x)
        n, c, h, w = x.shape
        if c % 4:
            raise ValueError('global_avgpool: C %% 4 != 0')
        y = new_nhwc(n, c, 1, 1, x.device)
        ws = _ws(call('ssg_sample_channel_sum_workspace_bytes', n, h * w, c), x.device)
        call('ssg_sample_channel_sum_f32', ptr(x), _ld(x), None, 0, n, h * w, c, 1.0 / (h * w), ptr(y), ptr(ws), stream_ptr())
        ctx.cfg = (n, c, h, w)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        n, c, h, w = ctx.cfg
        dy = to_nhwc(dy)
        if _ld(dy) != c:                            # the kernel reads the pooled gradient as dense [N][C] rows
            raise ValueError('global_avgpool: gradient rows are %d floats apart, %d expected' % (_ld(dy), c))
        dx = new_nhwc(n, c, h, w, dy.device)
        call('ssg_broadcast_rows_f32', ptr(dy), n, h * w, c, 1.0 / (h * w), ptr(dx), _ld(dx), stream_ptr())
        return dx


def global_avgpool(x):
    """F.adaptive_avg_pool2d(x, 1) -> [N, C, 1, 1]."""
    _lib.require_gpu(x)
    return _GlobalAvgPool.apply(x)


class _SEGate(torch.autograd.Function):
    """sigmoid(_se_expand(swish(_se_reduce(sq)))) on the pooled [N, C, 1, 1] vector (efficientnet_pytorch/model.py:84-86) as
    2 kernels forward and 3 backward (csrc/se_gate.hip) instead of two 1x1 conv launches with their packs, activations,
    split-K slabs and reducers."""

    @staticmethod
    def forward(ctx, sq, w1, b1, w2, b2):
        sq = to_nhwc(sq)
        n, c = sq.shape[0], sq.shape[1]
        s_ = w1.shape[0]
        dev = sq.device
        w1c = w1.detach().reshape(s_, c).contiguous(); w2c = w2.detach().reshape(c, s_).contiguous()
        h_pre = torch.empty((n, s_), dtype=torch.float32, device=dev)
        gate = new_nhwc(n, c, 1, 1, dev)
        tmp = torch.empty(call('ssg_se_gate_workspace_floats', n, c, s_), dtype=torch.float32, device=dev)
        call('ssg_se_gate_fwd_f32', ptr(sq), _ld(sq), n, c, ptr(w1c), ptr(b1.detach()) if b1 is not None else None, ptr(w2c),
             ptr(b2.detach()) if b2 is not None else None, s_, ptr(h_pre), ptr(gate), _ld(gate), ptr(tmp), stream_ptr())
        ctx.save_for_backward(sq, w1c, w2c, h_pre, gate)
        ctx.cfg = (n, c, s_, tuple(w1.shape), tuple(w2.shape), b1 is not None, b2 is not None)
        return gate

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dgate):
        sq, w1c, w2c, h_pre, gate = ctx.saved_tensors
        n, c, s_, shp1, shp2, has_b1, has_b2 = ctx.cfg
        dev = sq.device
        dgate = to_nhwc(dgate)
        dsq = new_nhwc(n, c, 1, 1, dev)
        dw1 = torch.empty((s_, c), dtype=torch.float32, device=dev); dw2 = torch.empty((c, s_), dtype=torch.float32, device=dev)
        db1 = torch.empty(s_, dtype=torch.float32, device=dev) if has_b1 else None
        db2 = torch.empty(c, dtype=torch.float32, device=dev) if has_b2 else None
        tmp = torch.empty(call('ssg_se_gate_workspace_floats', n, c, s_), dtype=torch.float32, device=dev)
        call('ssg_se_gate_bwd_f32', ptr(dgate), _ld(dgate), ptr(gate), _ld(gate), ptr(h_pre), ptr(sq), _ld(sq), n, c, ptr(w1c), ptr(w2c), s_,
             ptr(dsq), _ld(dsq), ptr(dw1), ptr(db1), ptr(dw2), ptr(db2), ptr(tmp), stream_ptr())
        return dsq, dw1.reshape(shp1), db1, dw2.reshape(shp2), db2


def se_gate(sq, reduce_conv, expand_conv):
    """The squeeze-excite gate for pooled `sq` [N, C, 1, 1] through the block's `_se_reduce` / `_se_expand` 1x1 conv modules;
    None when the shape is outside the fused kernels' range (the caller then runs the convs)."""
    _lib.require_gpu(sq)
    w1 = param('se_gate', 'reduce_conv.weight', reduce_conv.weight, sq, packed=True)      # (the node reads dense reshapes of both)
    w2 = param('se_gate', 'expand_conv.weight', expand_conv.weight, sq, packed=True)
    b1 = param('se_gate', 'reduce_conv.bias', reduce_conv.bias, sq)
    b2 = param('se_gate', 'expand_conv.bias', expand_conv.bias, sq)
    n, c = sq.shape[0], sq.shape[1]
    if tuple(w1.shape[1:]) != (c, 1, 1) or tuple(w2.shape) != (c, w1.shape[0], 1, 1) or sq.dtype != torch.float32:
        return None
    if not call('ssg_se_gate_ok', n, c, w1.shape[0]):
        return None
    return _SEGate.apply(sq, w1, b1, w2, b2)


class _ChannelScale(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, s):
        x = to_nhwc(x); s = to_nhwc(s)
        n, c, h, w = x.shape
        if tuple(s.shape) != (n, c, 1, 1) or c % 4:
            raise ValueError('channel_scale: gate %s does not match %s' % (tuple(s.shape), tuple(x.shape)))
        if _ld(s) != c:                             # the kernels read the gate as dense [N][C] rows
            raise ValueError('channel_scale: gate rows are %d floats apart, %d expected' % (_ld(s), c))
        y = new_nhwc(n, c, h, w, x.device)
        call('ssg_channel_scale_fwd_f32', ptr(x), _ld(x), ptr(s), n, h * w, c, ptr(y), _ld(y), stream_ptr())
        ctx.save_for_backward(x, s)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, s = ctx.saved_tensors
        dy = to_nhwc(dy)
        n, c, h, w = x.shape
        dx = new_nhwc(n, c, h, w, x.device)
        call('ssg_channel_scale_fwd_f32', ptr(dy), _ld(dy), ptr(s), n, h * w, c, ptr(dx), _ld(dx), stream_ptr())
        ds = new_nhwc(n, c, 1, 1, x.device)
        ws = _ws(call('ssg_sample_channel_sum_workspace_bytes', n, h * w, c), x.device)
        call('ssg_sample_channel_sum_f32', ptr(dy), _ld(dy), ptr(x), _ld(x), n, h * w, c, 1.0, ptr(ds), ptr(ws), stream_ptr())
        return dx, ds


def channel_scale(x, s):
    """x * s with s of shape [N, C, 1, 1] (squeeze-excite gate, drop-connect mask)."""
    _lib.require_gpu(x)
    return _ChannelScale.apply(x, s)


# ----------------------------------------------------------------------------- spectral norm (unwired row A12)
class _SpectralNormWeight(torch.autograd.Function):
    @staticmethod
    def forward(ctx, weight, u, v, n_iter, eps):
        wm = weight.contiguous()
        rows = wm.shape[0]
        cols = wm.numel() // rows
        out = torch.empty_like(wm)
        sigma = torch.empty((), dtype=torch.float32, device=wm.device)
        ws = _ws(call('ssg_spectral_norm_workspace_bytes', rows, cols), wm.device)
        call('ssg_spectral_norm_fwd_f32', ptr(wm), rows, cols, ptr(u), ptr(v), n_iter, float(eps), ptr(out), ptr(sigma), ptr(ws), stream_ptr())
        # the reference clones u, v after the in-place iteration so backward sees this call's vectors
        ctx.save_for_backward(wm, u.clone(), v.clone(), sigma)
        ctx.mark_non_differentiable(sigma)
        return out, sigma

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dwsn, _):
        wm, u, v, sigma = ctx.saved_tensors
        rows = wm.shape[0]
        cols = wm.numel() // rows
        dwsn = dwsn.contiguous()
        dw = torch.empty_like(wm)
        ws = _ws(call('ssg_spectral_norm_workspace_bytes', rows, cols), wm.device)
        call('ssg_spectral_norm_bwd_f32', ptr(dwsn), ptr(wm), rows, cols, ptr(u), ptr(v), ptr(sigma), ptr(dw), ptr(ws), stream_ptr())
        return dw, None, None, None, None


class _Conv2dSN(torch.autograd.Function):
    """conv2d(x, weight_orig / sigma) (+bias, +activation) with the spectral norm INSIDE the conv: one in-place power iteration
    on (u, v) -> sigma (spectral_norm.py:73-88), then weight_orig is packed with 1/sigma for the forward and the input
    gradient.  W / sigma is never written out, nothing of the weight is cached across forwards (sigma moves every training
    forward), and the weight gradient is mapped back through dW = dWsn/sigma - (sum(dWsn . W)/sigma^2) u v^T."""

    @staticmethod
    def forward(ctx, x, weight_orig, u, v, bias, stride, pad, act, slope, n_iter, eps):
        x = to_nhwc(x)
        wm = weight_orig.contiguous()
        rows = wm.shape[0]
        cols = wm.numel() // rows
        sigma = torch.empty((), dtype=torch.float32, device=wm.device)
        ws = _ws(call('ssg_spectral_norm_workspace_bytes', rows, cols), wm.device)
        call('ssg_spectral_norm_fwd_f32', ptr(wm), rows, cols, ptr(u), ptr(v), n_iter, float(eps), None, ptr(sigma), ptr(ws), stream_ptr())
        y = _conv_fwd_impl(x, None, wm, bias, stride, pad, act, slope, wscale=sigma)
        ctx.save_for_backward(x, wm, u.clone(), v.clone(), sigma, y if act != ACT_NONE else None)
        ctx.cfg = (stride, pad, act, slope, bias is not None)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, wm, u, v, sigma, y = ctx.saved_tensors
        stride, pad, act, slope, has_bias = ctx.cfg
        dy = to_nhwc(dy)
        if act != ACT_NONE:
            dy = _act_bwd(y, dy, act, slope)
        n, c1, h, w = x.shape
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = _conv_dgrad_impl(dy, wm, stride, pad, h, w, 0, c1, wscale=sigma)
        if ctx.needs_input_grad[1]:
            dwsn = _conv_wgrad_impl(x, None, dy, wm.shape, stride, pad)
            rows = wm.shape[0]
            cols = wm.numel() // rows
            dw = torch.empty_like(wm)
            ws = _ws(call('ssg_spectral_norm_workspace_bytes', rows, cols), wm.device)
            call('ssg_spectral_norm_bwd_f32', ptr(dwsn), ptr(wm), rows, cols, ptr(u), ptr(v), ptr(sigma), ptr(dw), ptr(ws), stream_ptr())
        if has_bias and ctx.needs_input_grad[4]:
            db = _channel_sum(dy, wm.shape[0])
        return dx, dw, None, None, db, None, None, None, None, None, None


def conv2d_sn(x, weight_orig, u, v, bias=None, stride=1, padding=0, act=ACT_NONE, slope=0.0, n_power_iterations=1, eps=1e-12):
    """Spectrally normalised conv2d: see _Conv2dSN.  `n_power_iterations = 0` in eval mode (no update of u, v)."""
    _lib.require_gpu(x)
    weight_orig = param('conv2d_sn', 'weight_orig', weight_orig, x, packed=True)      # (the node reads weight_orig.contiguous())
    u = param('conv2d_sn', 'u', u, x, written=True)
    v = param('conv2d_sn', 'v', v, x, written=True)
    bias = param('conv2d_sn', 'bias', bias, x)
    pad = tuple(int(p) for p in padding) if isinstance(padding, (tuple, list)) else int(padding)
    return _Conv2dSN.apply(x, weight_orig, u, v, bias, int(stride), pad, int(act), float(slope), int(n_power_iterations), float(eps))


def spectral_norm_weight(weight_orig, u, v, n_power_iterations=1, eps=1e-12):
    """weight_orig / sigma after `n_power_iterations` in-place power-iteration updates of u, v."""
    weight_orig = param('spectral_norm_weight', 'weight_orig', weight_orig, None, packed=True)      # (the node reads weight_orig.contiguous())
    u = param('spectral_norm_weight', 'u', u, weight_orig, written=True)
    v = param('spectral_norm_weight', 'v', v, weight_orig, written=True)
    return _SpectralNormWeight.apply(weight_orig, u, v, int(n_power_iterations), float(eps))


class _Add(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        a = to_nhwc(a); b = to_nhwc(b)
        n, c, h, w = a.shape
        if _ld(a) != _ld(b) or a.shape != b.shape:
            raise ValueError('add: shape/stride mismatch')
        if _ld(a) != pad4(c):                       # whole pixel rows are added: a channel slice would read its neighbours' lanes
            raise ValueError('add: pixel stride %d is wider than the %d channels (channel slice of another tensor)' % (_ld(a), c))
        y = new_nhwc(n, c, h, w, a.device, ld=_ld(a))
        call('ssg_add_f32', ptr(a), ptr(b), n * h * w * _ld(a), ptr(y), stream_ptr())
        return y

    @staticmethod
    def backward(ctx, g):
        return g, g


def add(a, b):
    """a + b for two NHWC tensors of the same shape."""
    _lib.require_gpu(a)
    return _Add.apply(a, b)


class _ConcatChannels(torch.autograd.Function):
    @staticmethod
    def forward(ctx, *xs):
        xs = [to_nhwc(x) for x in xs]
        n, _, h, w = xs[0].shape
        cs = [x.shape[1] for x in xs]
        if any(c % 4 for c in cs):
            raise ValueError('concat_channels: every input needs C %% 4 == 0 (got %s)' % cs)
        y = new_nhwc(n, sum(cs), h, w, xs[0].device)
        off = 0
        for x, c in zip(xs, cs):
            dst = y[:, off:off + c]
            call('ssg_copy_channels_f32', ptr(x), _ld(x), n * h * w, c, ptr(dst), _ld(y), stream_ptr())
            off += c
        ctx.cs = cs
        return y

    @staticmethod
    def backward(ctx, g):
        outs, off = [], 0
        for c in ctx.cs:
            outs.append(g[:, off:off + c])
            off += c
        return tuple(outs)


def concat_channels(*xs):
    """torch.cat(xs, 1) materialised (only needed for more than two inputs; convs take two pointers)."""
    _lib.require_gpu(xs[0])
    return xs[0] if len(xs) == 1 else _ConcatChannels.apply(*xs)
