"""CPU: the launch decisions of the conv dispatcher (conv_igemm.hip plan_conv, conv_wgrad.hip make_plan), pinned.

Every row builds the descriptor that ops._conv_launch / ops._conv_wgrad_impl would build for one launch, with dummy
16-byte-aligned addresses, and asks the library's host-side queries in the order ops.py asks them.  Nothing is launched or
dereferenced.  Rows: every distinct conv / input-gradient / weight-gradient launch of the 16 x 512^2 step
(profiles/r04_a_shapes_per_launch.txt) plus the edges of the dispatch (split-K grids, narrow outputs, merged parity, thin and
1x1 shapes, concat inputs, misaligned outputs, fused input transform, backward statistics, fp32 MFMA, the k32 modes)."""
import ctypes

import pytest

A = 1 << 32                                 # dummy addresses: 16-byte aligned, distinct, never dereferenced
IN1, IN2, W, BIAS, RES, OUT, PART, WS, WSPLIT, SCALE, SHIFT, BX, MEAN, DW = (A * (k + 1) for k in range(14))
ACT_NONE, ACT_RELU = 0, 1


def _pad4(c):
    return (c + 3) // 4 * 4


def _opt(opts, key, default=None):
    for o in opts.split():
        if o == key:
            return True
        if o.startswith(key + '='):
            return int(o.split('=')[1])
    return default


def _classes(k, s, p):
    """(py, px, taps) per output parity class of a strided input gradient, as ops._conv_dgrad_impl lists them."""
    out = []
    for py in range(s):
        for px in range(s):
            out.append((py, px, [((py + p - ky) // s, (px + p - kx) // s) for ky in range(k) for kx in range(k)
                                 if (py + p - ky) % s == 0 and (px + p - kx) % s == 0]))
    return out


def _conv_desc(lib, spec):
    """ssg_conv_desc of one launch.  spec = (op, n, c1, c2, h, w, cout, k, stride, opts); h x w is the forward conv's input.
    fwd: x [c1 + c2] -> y [cout].  dgrad: dy [c1] -> dx [cout] (stride 1, or `parity` = the merged launch of stride 2, or
    `class=py,px` = one parity class).  opts: bias res relu (epilogue), mis (out 4 bytes off 16, odd ldo)."""
    op, n, c1, c2, h, w, cout, k, s, opts = spec
    p = k // 2
    oh, ow = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
    d = lib.ConvDesc()
    d.in1 = IN1; d.C1 = _pad4(c1); d.ld1 = _pad4(c1)
    if c2:
        d.in2 = IN2; d.C2 = _pad4(c2); d.ld2 = _pad4(c2)
    cred = d.C1 + d.C2
    if op == 'fwd':
        taps = [(ky - p, kx - p) for ky in range(k) for kx in range(k)]
        d.N, d.H, d.W = n, h, w
        d.GH, d.GW, d.OH, d.OW = oh, ow, oh, ow
        d.in_sy = d.in_sx = s; d.out_sy = d.out_sx = 1
    else:
        d.N, d.H, d.W = n, oh, ow
        d.OH, d.OW = h, w
        d.in_sy = d.in_sx = 1
        if s == 1:
            taps = [(p - ky, p - kx) for ky in range(k) for kx in range(k)]
            d.GH, d.GW = h, w; d.out_sy = d.out_sx = 1
        elif _opt(opts, 'parity'):
            taps = [t for _, _, ts in _classes(k, s, p) for t in ts]
            d.GH, d.GW = (h + 1) // 2, (w + 1) // 2; d.out_sy = d.out_sx = s; d.parity_merge = 1
        else:
            py, px = divmod(_opt(opts, 'class'), 2)
            taps = _classes(k, s, p)[2 * py + px][2]
            d.GH, d.GW = (h - py + s - 1) // s, (w - px + s - 1) // s
            d.out_sy = d.out_sx = s; d.out_oy, d.out_ox = py, px
    kmode = 0 if cred % 16 == 0 and d.C1 % 16 == 0 else 1
    d.Kp = len(taps) * cred if kmode == 0 else (len(taps) * cred + 15) // 16 * 16
    d.w = W; d.kmode = kmode
    d.ntaps = len(taps)
    for t, (dy, dx) in enumerate(taps):
        d.dy[t] = dy; d.dx[t] = dx
    d.bias = BIAS if _opt(opts, 'bias') else None
    if _opt(opts, 'res'):
        d.res = RES; d.ldr = _pad4(cout)
    d.act = ACT_RELU if _opt(opts, 'relu') else ACT_NONE
    d.out = OUT + 4 if _opt(opts, 'mis') else OUT
    d.Cout = cout; d.ldo = _pad4(cout) + 1 if _opt(opts, 'mis') else _pad4(cout)
    return d


def conv_row(lib, labels, spec):
    """(label, split_bn, bnpart_rows, workspace_bytes, in_affine_ok, bwd_stats_ok) of one launch, queried as ops._conv_launch
    does: the split pack first (opts without `fp32`: SSG_MFMA_SPLIT=1), then the fused input transform (`aff`) / backward
    statistics (`bwd`), the statistics rows (`bn`: wanted), the split-K workspace.  label = 'declined' where _conv_launch
    declines; workspace_bytes = None where it does not ask."""
    opts = spec[-1]
    d = _conv_desc(lib, spec)
    q = lambda name: lib.call(name, ctypes.byref(d))
    split = q('ssg_conv2d_split_bn') if not _opt(opts, 'fp32') and d.kmode == 0 else 0
    if split:
        d.w_split = WSPLIT
    if _opt(opts, 'aff'):
        d.in_scale = SCALE; d.in_shift = SHIFT; d.in_act = ACT_RELU
    if _opt(opts, 'bwd'):
        d.bwd_x = BX; d.bwd_ldx = _pad4(spec[6]); d.bwd_scale = SCALE; d.bwd_shift = SHIFT; d.bwd_mean = MEAN
        d.bwd_act = ACT_RELU
    aff, bwd = q('ssg_conv2d_in_affine_ok'), q('ssg_conv2d_bwd_stats_ok')
    rows = q('ssg_conv2d_bnpart_rows')
    declined = ((d.parity_merge and split != 64) or (_opt(opts, 'aff') and not (split and aff))
                or (_opt(opts, 'bwd') and not (split and bwd and rows)))
    if rows and (_opt(opts, 'bn') or _opt(opts, 'bwd')) and not declined:
        d.bnpart = PART
    ws = None
    if not d.bnpart and not split:
        ws = q('ssg_conv2d_workspace_bytes')
        if ws:
            d.ws = WS; d.ws_bytes = ws
    label = 'declined' if declined else labels.get(q('ssg_conv2d_kernel_id'), '?') + ('+splitk' if d.ws else '')
    return (label, split, rows, ws, aff, bwd)


def wgrad_row(lib, labels, spec):
    """(label, workspace_bytes, in_affine_ok) of one weight-gradient launch, queried as ops._conv_wgrad_impl does.
    spec = ('wgrad', n, c1, c2, h, w, cout, k, stride, opts); opts: fp32 (flags 0), aff (fused input transform)."""
    _, n, c1, c2, h, w, cout, k, s, opts = spec
    p = k // 2
    d = lib.WgradDesc()
    d.in1 = IN1; d.C1 = _pad4(c1); d.ld1 = _pad4(c1)
    if c2:
        d.in2 = IN2; d.C2 = _pad4(c2); d.ld2 = _pad4(c2)
    d.N, d.H, d.W = n, h, w
    d.dout = OUT; d.Cout = cout; d.ldd = _pad4(cout)
    d.GH, d.GW = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
    d.in_sy = d.in_sx = s
    d.ntaps = k * k
    for t in range(k * k):
        d.ky[t], d.kx[t] = divmod(t, k)
        d.dy[t], d.dx[t] = d.ky[t] - p, d.kx[t] - p
    d.KH = d.KW = k; d.Cin_real = c1 + c2
    d.dw_oihw = DW
    d.flags = 0 if _opt(opts, 'fp32') else 1
    aff = None
    if _opt(opts, 'aff'):
        d.in_scale = SCALE; d.in_shift = SHIFT; d.in_act = ACT_RELU
        aff = lib.call('ssg_conv2d_wgrad_in_affine_ok', ctypes.byref(d))
        if not aff:
            return ('declined', None, aff)
    nbytes = lib.call('ssg_conv2d_wgrad_workspace_bytes', ctypes.byref(d))
    d.ws = WS; d.ws_bytes = nbytes
    return (labels.get(lib.call('ssg_conv2d_wgrad_kernel_id', ctypes.byref(d)), '?'), nbytes, aff)


def run_row(lib, labels, wlabels, spec):
    """Set the k32 modes a row asks for (opts k32=0/1/2, wk32=0/1), restored to the default (1) afterwards."""
    opts = spec[-1]
    lib.call('ssg_conv_set_k32_mode', _opt(opts, 'k32', 1))
    lib.call('ssg_wgrad_set_k32_mode', _opt(opts, 'wk32', 1))
    try:
        return wgrad_row(lib, wlabels, spec) if spec[0] == 'wgrad' else conv_row(lib, labels, spec)
    finally:
        lib.call('ssg_conv_set_k32_mode', 1)
        lib.call('ssg_wgrad_set_k32_mode', 1)


# expected: (label, split_bn, bnpart_rows, workspace_bytes, in_affine_ok, bwd_stats_ok) per conv launch, (label, workspace_bytes,
# in_affine_ok) per weight gradient
ROWS = [
    (('fwd', 16, 64, 0, 512, 512, 64, 3, 1, 'bn'), ('conv_halo_k32_kernel<16,64>', 1064, 8192, None, 0, 1)),
    (('dgrad', 16, 64, 0, 512, 512, 64, 3, 1, ''), ('conv_halo_k32_kernel<16,64>', 1064, 8192, None, 0, 1)),
    (('fwd', 16, 256, 0, 128, 128, 256, 3, 1, 'bn'), ('conv_halo_k32_kernel<8,128>', 1128, 1024, None, 1, 1)),
    (('dgrad', 16, 256, 0, 128, 128, 256, 3, 1, ''), ('conv_halo_k32_kernel<8,128>', 1128, 1024, None, 1, 1)),
    (('fwd', 16, 128, 0, 256, 256, 128, 3, 1, 'bn'), ('conv_halo_k32_kernel<8,128>', 1128, 4096, None, 1, 1)),
    (('dgrad', 16, 128, 0, 256, 256, 128, 3, 1, ''), ('conv_halo_k32_kernel<8,128>', 1128, 4096, None, 1, 1)),
    (('fwd', 16, 192, 0, 512, 512, 64, 3, 1, 'bn'), ('conv_halo_k32_kernel<16,64>', 1064, 8192, None, 0, 1)),
    (('dgrad', 16, 192, 0, 512, 512, 64, 3, 1, ''), ('conv_halo_k32_kernel<16,64>', 1064, 8192, None, 0, 1)),
    (('wgrad', 16, 192, 0, 512, 512, 64, 3, 1, ''), ('wgrad_k32_kernel<64,64>', 452984832, None)),
    (('wgrad', 16, 384, 0, 256, 256, 128, 3, 1, ''), ('wgrad_k32_kernel<64,64>', 452984832, None)),
    (('fwd', 16, 384, 0, 64, 64, 384, 3, 1, 'bn'), ('conv_halo_k32_kernel<8,128>', 1128, 256, None, 1, 1)),
    (('dgrad', 16, 384, 0, 64, 64, 384, 3, 1, ''), ('conv_halo_k32_kernel<8,128>', 1128, 256, None, 1, 1)),
    (('fwd', 16, 384, 0, 256, 256, 128, 3, 1, 'bn'), ('conv_halo_k32_kernel<8,128>', 1128, 4096, None, 1, 1)),
    (('dgrad', 16, 384, 0, 256, 256, 128, 3, 1, ''), ('conv_halo_k32_kernel<8,128>', 1128, 4096, None, 1, 1)),
    (('fwd', 16, 64, 0, 512, 512, 128, 3, 1, 'bn'), ('conv_halo_k32_kernel<8,128>', 1128, 16384, None, 1, 1)),
    (('dgrad', 16, 64, 0, 512, 512, 128, 3, 1, ''), ('conv_halo_k32_kernel<8,128>', 1128, 16384, None, 1, 1)),
    (('fwd', 16, 64, 0, 256, 256, 128, 3, 1, 'bn'), ('conv_halo_k32_kernel<8,128>', 1128, 4096, None, 1, 1)),
    (('dgrad', 16, 64, 0, 256, 256, 128, 3, 1, ''), ('conv_halo_k32_kernel<8,128>', 1128, 4096, None, 1, 1)),
    (('fwd', 16, 128, 0, 256, 256, 64, 3, 1, 'bn'), ('conv_halo_k32_kernel<16,64>', 1064, 2048, None, 0, 1)),
    (('dgrad', 16, 128, 0, 256, 256, 64, 3, 1, ''), ('conv_halo_k32_kernel<16,64>', 1064, 2048, None, 0, 1)),
    (('fwd', 16, 128, 0, 256, 256, 256, 3, 1, 'bn'), ('conv_halo_k32_kernel<8,128>', 1128, 4096, None, 1, 1)),
    (('dgrad', 16, 128, 0, 256, 256, 256, 3, 1, ''), ('conv_halo_k32_kernel<8,128>', 1128, 4096, None, 1, 1)),
    (('wgrad', 16, 64, 0, 256, 256, 128, 3, 1, ''), ('wgrad_k32_kernel<64,64>', 150994944, None)),
    (('wgrad', 16, 128, 0, 128, 128, 256, 3, 1, ''), ('wgrad_k32_kernel<64,64>', 150994944, None)),
    (('fwd', 16, 128, 0, 128, 128, 256, 3, 1, 'bn'), ('conv_halo_k32_kernel<8,128>', 1128, 1024, None, 1, 1)),
    (('dgrad', 16, 128, 0, 128, 128, 256, 3, 1, ''), ('conv_halo_k32_kernel<8,128>', 1128, 1024, None, 1, 1)),
    (('wgrad', 16, 512, 0, 128, 128, 256, 3, 1, ''), ('wgrad_k32_kernel<64,64>', 301989888, None)),
    (('wgrad', 16, 64, 0, 512, 512, 64, 3, 1, ''), ('wgrad_k32_kernel<64,64>', 150994944, None)),
    (('wgrad', 16, 256, 0, 128, 128, 256, 3, 1, ''), ('wgrad_k32_kernel<64,64>', 150994944, None)),
    (('wgrad', 16, 128, 0, 256, 256, 128, 3, 1, ''), ('wgrad_k32_kernel<64,64>', 150994944, None)),
    (('fwd', 16, 256, 0, 128, 128, 128, 3, 1, 'bn'), ('conv_halo_k32_kernel<8,128>', 1128, 1024, None, 1, 1)),
    (('dgrad', 16, 256, 0, 128, 128, 128, 3, 1, ''), ('conv_halo_k32_kernel<8,128>', 1128, 1024, None, 1, 1)),
    (('fwd', 16, 512, 0, 128, 128, 256, 3, 1, 'bn'), ('conv_halo_k32_kernel<8,128>', 1128, 1024, None, 1, 1)),
    (('dgrad', 16, 512, 0, 128, 128, 256, 3, 1, ''), ('conv_halo_k32_kernel<8,128>', 1128, 1024, None, 1, 1)),
    (('wgrad', 16, 64, 0, 512, 512, 64, 3, 2, ''), ('wgrad_dma_x3_kernel<128,64>', 30081024, None)),
    (('fwd', 16, 128, 0, 512, 512, 4, 3, 1, 'bn'), ('thin4_cout_kernel', 0, 0, 0, 0, 0)),
    (('dgrad', 16, 128, 0, 512, 512, 4, 3, 1, ''), ('thin4_cout_kernel', 0, 0, 0, 0, 0)),
    (('wgrad', 16, 256, 0, 64, 64, 512, 3, 1, ''), ('wgrad_k32_kernel<64,64>', 150994944, None)),
    (('dgrad', 16, 64, 0, 512, 512, 64, 3, 2, 'parity'), ('conv_igemm_halo_x3_kernel<128,64,4,1,true>', 64, 8192, None, 0, 0)),
    (('fwd', 16, 256, 0, 64, 64, 512, 3, 1, 'bn'), ('conv_halo_k32_kernel<8,128>', 1128, 256, None, 1, 1)),
    (('dgrad', 16, 256, 0, 64, 64, 512, 3, 1, ''), ('conv_halo_k32_kernel<8,128>', 1128, 256, None, 1, 1)),
    (('fwd', 16, 512, 0, 128, 128, 16, 3, 1, 'bn'), ('conv_halo_k32_kernel<8,16>', 1016, 1024, None, 0, 0)),
    (('dgrad', 16, 512, 0, 128, 128, 16, 3, 1, ''), ('conv_halo_k32_kernel<8,16>', 1016, 1024, None, 0, 0)),
    (('fwd', 16, 3, 0, 512, 512, 64, 3, 1, 'bn'), ('thin32_cin_kernel', 0, 0, 0, 0, 0)),
    (('dgrad', 16, 3, 0, 512, 512, 64, 3, 1, ''), ('thin32_cin_kernel', 0, 0, 0, 0, 0)),
    (('wgrad', 16, 128, 0, 256, 256, 128, 3, 2, ''), ('wgrad_dma_x3_kernel<128,128>', 66650112, None)),
    (('wgrad', 16, 512, 0, 64, 64, 512, 3, 2, ''), ('wgrad_dma_x3_kernel<128,128>', 66060288, None)),
    (('wgrad', 16, 256, 0, 128, 128, 256, 3, 2, ''), ('wgrad_dma_x3_kernel<128,128>', 66060288, None)),
    (('fwd', 16, 512, 0, 64, 64, 256, 3, 1, 'bn'), ('conv_halo_k32_kernel<8,128>', 1128, 256, None, 1, 1)),
    (('dgrad', 16, 512, 0, 64, 64, 256, 3, 1, ''), ('conv_halo_k32_kernel<8,128>', 1128, 256, None, 1, 1)),
    (('fwd', 16, 512, 0, 32, 32, 512, 3, 1, 'bn'), ('conv_halo_k32_kernel<8,128>', 1128, 64, None, 1, 1)),
    (('dgrad', 16, 512, 0, 32, 32, 512, 3, 1, ''), ('conv_halo_k32_kernel<8,128>', 1128, 64, None, 1, 1)),
    (('fwd', 16, 64, 0, 512, 512, 3, 3, 1, 'bn'), ('thin4_cout_kernel', 0, 0, 0, 0, 0)),
    (('dgrad', 16, 64, 0, 512, 512, 3, 3, 1, ''), ('thin4_cout_kernel', 0, 0, 0, 0, 0)),
    (('fwd', 16, 64, 0, 512, 512, 64, 3, 2, 'bn'), ('conv_igemm_dma_x3_kernel<64>', 64, 8192, None, 0, 0)),
    (('wgrad', 16, 768, 0, 64, 64, 384, 3, 1, ''), ('wgrad_k32_kernel<64,64>', 222953472, None)),
    (('dgrad', 16, 128, 0, 256, 256, 128, 3, 2, 'parity'), ('conv_igemm_halo_x3_kernel<128,64,4,1,true>', 64, 2048, None, 0, 0)),
    (('wgrad', 16, 3, 0, 512, 512, 64, 3, 1, ''), ('wgrad32_cin_kernel', 18874368, None)),
    (('wgrad', 16, 384, 0, 64, 64, 384, 3, 1, ''), ('wgrad_k32_kernel<64,64>', 185794560, None)),
    (('fwd', 16, 256, 0, 256, 256, 8, 3, 1, 'bn'), ('thin4_cout_kernel', 0, 0, 0, 0, 0)),
    (('dgrad', 16, 256, 0, 256, 256, 8, 3, 1, ''), ('thin4_cout_kernel', 0, 0, 0, 0, 0)),
    (('wgrad', 16, 4, 0, 512, 512, 128, 3, 1, ''), ('wgrad32_cin_kernel', 18874368, None)),
    (('dgrad', 16, 256, 0, 128, 128, 256, 3, 2, 'parity'), ('conv_igemm_halo_x3_kernel<128,64,4,1,true>', 64, 512, None, 0, 0)),
    (('fwd', 16, 128, 0, 256, 256, 128, 3, 2, 'bn'), ('conv_igemm_dma_x3_kernel<128>', 128, 2048, None, 0, 0)),
    (('wgrad', 16, 192, 0, 512, 512, 64, 1, 1, ''), ('wgrad_dma_x3_kernel<128,64>', 25165824, None)),
    (('fwd', 16, 256, 0, 128, 128, 256, 3, 2, 'bn'), ('conv_igemm_dma_x3_kernel<128>', 128, 512, None, 0, 0)),
    (('dgrad', 16, 512, 0, 64, 64, 512, 3, 2, 'parity'), ('conv_igemm_halo_x3_kernel<128,64,4,1,true>', 64, 128, None, 0, 0)),
    (('fwd', 16, 768, 0, 64, 64, 384, 3, 1, 'bn'), ('conv_halo_k32_kernel<8,128>', 1128, 256, None, 0, 1)),
    (('dgrad', 16, 768, 0, 64, 64, 384, 3, 1, ''), ('conv_halo_k32_kernel<8,128>', 1128, 256, None, 0, 1)),
    (('fwd', 16, 512, 0, 64, 64, 512, 3, 2, 'bn'), ('conv_igemm_dma_x3_kernel<128>', 128, 128, None, 0, 0)),
    (('wgrad', 16, 64, 0, 512, 512, 3, 3, 1, ''), ('wgrad4_kernel<thin_cout>', 14155776, None)),
    (('wgrad', 16, 8, 0, 256, 256, 256, 3, 1, ''), ('wgrad_dma_x3_kernel<128,128>', 37748736, None)),
    (('wgrad', 16, 16, 0, 128, 128, 512, 3, 1, ''), ('wgrad_dma_x3_kernel<128,128>', 37748736, None)),
    (('fwd', 16, 768, 0, 64, 64, 24, 3, 1, 'bn'), ('conv_halo_k32_kernel<8,32>', 1032, 256, None, 0, 0)),
    (('dgrad', 16, 768, 0, 64, 64, 24, 3, 1, ''), ('conv_halo_k32_kernel<8,32>', 1032, 256, None, 0, 0)),
    (('fwd', 16, 192, 0, 512, 512, 64, 1, 1, 'bn'), ('conv_igemm_dma_x3_kernel<64>', 64, 32768, None, 0, 0)),
    (('wgrad', 16, 512, 0, 32, 32, 512, 3, 1, ''), ('wgrad_k32_kernel<64,64>', 150994944, None)),
    (('wgrad', 16, 384, 0, 256, 256, 128, 1, 1, ''), ('wgrad_dma_x3_kernel<128,128>', 66846720, None)),
    (('fwd', 16, 64, 0, 512, 512, 128, 1, 1, 'bn'), ('conv_igemm_dma_kernel<128,64>', 0, 32768, None, 0, 0)),
    (('fwd', 16, 128, 0, 256, 256, 256, 1, 1, 'bn'), ('conv_igemm_dma_x3_kernel<128>', 128, 8192, None, 0, 0)),
    (('wgrad', 16, 1024, 0, 32, 32, 512, 3, 1, ''), ('wgrad_k32_kernel<64,64>', 150994944, None)),
    (('fwd', 16, 384, 0, 256, 256, 128, 1, 1, 'bn'), ('conv_igemm_dma_x3_kernel<128>', 128, 8192, None, 0, 0)),
    (('fwd', 16, 768, 0, 16, 16, 768, 3, 1, 'bn'), ('conv_igemm_halo16_kernel<128,128>+splitk', 0, 0, 50331648, 0, 0)),
    (('dgrad', 16, 768, 0, 16, 16, 768, 3, 1, ''), ('conv_igemm_halo16_kernel<128,128>+splitk', 0, 0, 50331648, 0, 0)),
    (('fwd', 16, 16, 0, 128, 128, 512, 3, 1, 'bn'), ('conv_igemm_halo_x3_kernel<128,128>', 128, 2048, None, 0, 0)),
    (('dgrad', 16, 16, 0, 128, 128, 512, 3, 1, ''), ('conv_igemm_halo_x3_kernel<128,128>', 128, 2048, None, 0, 0)),
    (('fwd', 16, 3, 0, 512, 512, 64, 1, 1, 'bn'), ('thin4_cin_kernel', 0, 0, 0, 0, 0)),
    (('fwd', 16, 128, 0, 256, 256, 3, 3, 1, 'bn'), ('thin4_cout_kernel', 0, 0, 0, 0, 0)),
    (('dgrad', 16, 128, 0, 256, 256, 3, 3, 1, ''), ('thin4_cout_kernel', 0, 0, 0, 0, 0)),
    (('wgrad', 16, 256, 0, 64, 64, 384, 3, 1, ''), ('wgrad_k32_kernel<64,64>', 148635648, None)),
    (('wgrad', 16, 128, 0, 256, 256, 3, 3, 1, ''), ('wgrad4_kernel<thin_cout>', 14155776, None)),
    (('fwd', 16, 1024, 0, 32, 32, 512, 3, 1, 'bn'), ('conv_halo_k32_kernel<8,128>', 1128, 64, None, 0, 1)),
    (('dgrad', 16, 1024, 0, 32, 32, 512, 3, 1, ''), ('conv_halo_k32_kernel<8,128>', 1128, 64, None, 0, 1)),
    (('fwd', 16, 256, 0, 128, 128, 256, 1, 1, 'bn'), ('conv_igemm_dma_x3_kernel<128>', 128, 2048, None, 0, 0)),
    (('wgrad', 16, 512, 0, 128, 128, 256, 1, 1, ''), ('wgrad_dma_x3_kernel<128,128>', 67108864, None)),
    (('fwd', 16, 24, 0, 64, 64, 768, 3, 1, 'bn'), ('conv_igemm_kernel<128,128>', 0, 0, 0, 0, 0)),
    (('dgrad', 16, 24, 0, 64, 64, 768, 3, 1, ''), ('conv_igemm_kernel<128,128>', 0, 0, 0, 0, 0)),
    (('fwd', 16, 64, 0, 512, 512, 64, 1, 1, 'bn'), ('conv_igemm_dma_kernel<128,64>', 0, 32768, None, 0, 0)),
    (('fwd', 16, 384, 0, 64, 64, 256, 3, 1, 'bn'), ('conv_halo_k32_kernel<8,128>', 1128, 256, None, 1, 1)),
    (('dgrad', 16, 384, 0, 64, 64, 256, 3, 1, ''), ('conv_halo_k32_kernel<8,128>', 1128, 256, None, 1, 1)),
    (('fwd', 16, 256, 0, 64, 64, 384, 3, 1, 'bn'), ('conv_halo_k32_kernel<8,128>', 1128, 256, None, 1, 1)),
    (('dgrad', 16, 256, 0, 64, 64, 384, 3, 1, ''), ('conv_halo_k32_kernel<8,128>', 1128, 256, None, 1, 1)),
    (('wgrad', 16, 24, 0, 64, 64, 768, 3, 1, ''), ('wgrad_dma_x3_kernel<128,128>', 55738368, None)),
    (('fwd', 16, 512, 0, 128, 128, 256, 1, 1, 'bn'), ('conv_igemm_dma_x3_kernel<128>', 128, 2048, None, 0, 0)),
    (('fwd', 16, 3, 0, 256, 256, 128, 3, 1, 'bn'), ('thin32_cin_kernel', 0, 0, 0, 0, 0)),
    (('dgrad', 16, 3, 0, 256, 256, 128, 3, 1, ''), ('thin32_cin_kernel', 0, 0, 0, 0, 0)),
    (('fwd', 16, 128, 0, 256, 256, 128, 1, 1, 'bn'), ('conv_igemm_dma_x3_kernel<128>', 128, 8192, None, 0, 0)),
    (('wgrad', 16, 3, 0, 512, 512, 4, 3, 1, ''), ('wgrad_tiny4_kernel', 589824, None)),
    (('wgrad', 16, 384, 0, 32, 32, 512, 3, 1, ''), ('wgrad_k32_kernel<64,64>', 184025088, None)),
    (('wgrad', 16, 768, 0, 16, 16, 768, 3, 1, ''), ('wgrad_halo_x3_kernel<32,128>', 148635648, None)),
    (('fwd', 16, 1024, 0, 32, 32, 32, 3, 1, 'bn'), ('conv_igemm_halo_kernel<128,64>+splitk', 0, 0, 12582912, 0, 0)),
    (('dgrad', 16, 1024, 0, 32, 32, 32, 3, 1, ''), ('conv_igemm_halo_kernel<128,64>+splitk', 0, 0, 12582912, 0, 0)),
    (('fwd', 16, 512, 0, 32, 32, 384, 3, 1, 'bn'), ('conv_igemm_halo_x3_kernel<128,64>', 64, 128, None, 0, 0)),
    (('dgrad', 16, 512, 0, 32, 32, 384, 3, 1, ''), ('conv_igemm_halo_x3_kernel<128,64>', 64, 128, None, 0, 0)),
    (('wgrad', 16, 768, 0, 64, 64, 384, 1, 1, ''), ('wgrad_dma_x3_kernel<128,128>', 66060288, None)),
    (('wgrad', 16, 64, 0, 256, 256, 128, 1, 1, ''), ('wgrad_dma_x3_kernel<128,128>', 16777216, None)),
    (('fwd', 16, 256, 0, 128, 128, 3, 3, 1, 'bn'), ('thin4_cout_kernel', 0, 0, 0, 0, 0)),
    (('dgrad', 16, 256, 0, 128, 128, 3, 3, 1, ''), ('thin4_cout_kernel', 0, 0, 0, 0, 0)),
    (('wgrad', 16, 256, 0, 128, 128, 3, 3, 1, ''), ('wgrad4_kernel<thin_cout>', 14155776, None)),
    (('wgrad', 16, 64, 0, 512, 512, 3, 1, 1, ''), ('wgrad4_kernel<thin_cout>', 1572864, None)),
    (('fwd', 16, 384, 0, 64, 64, 384, 1, 1, 'bn'), ('conv_igemm_dma_x3_kernel<128>', 128, 512, None, 0, 0)),
    (('fwd', 1, 1024, 0, 1, 16, 18432, 1, 1, 'bn'), ('conv_igemm_dma_kernel<128,128>', 0, 1, None, 0, 0)),
    (('fwd', 16, 512, 0, 16, 16, 768, 3, 1, 'bn'), ('conv_igemm_halo16_kernel<128,128>+splitk', 0, 0, 50331648, 0, 0)),
    (('dgrad', 16, 512, 0, 16, 16, 768, 3, 1, ''), ('conv_igemm_halo16_kernel<128,128>+splitk', 0, 0, 50331648, 0, 0)),
    (('fwd', 16, 64, 0, 512, 512, 3, 1, 1, 'bn'), ('thin4_cout_kernel', 0, 0, 0, 0, 0)),
    (('fwd', 16, 768, 0, 16, 16, 512, 3, 1, 'bn'), ('conv_igemm_halo16_kernel<128,128>+splitk', 0, 0, 50331648, 0, 0)),
    (('dgrad', 16, 768, 0, 16, 16, 512, 3, 1, ''), ('conv_igemm_halo16_kernel<128,128>+splitk', 0, 0, 50331648, 0, 0)),
    (('wgrad', 16, 512, 0, 16, 16, 768, 3, 1, ''), ('wgrad_halo_x3_kernel<32,128>', 141557760, None)),
    (('fwd', 16, 64, 0, 256, 256, 128, 1, 1, 'bn'), ('conv_igemm_dma_kernel<128,64>', 0, 8192, None, 0, 0)),
    (('wgrad', 16, 3, 0, 512, 512, 64, 1, 1, ''), ('wgrad4_kernel<thin_cin>', 2097152, None)),
    (('fwd', 16, 768, 0, 64, 64, 384, 1, 1, 'bn'), ('conv_igemm_dma_x3_kernel<128>', 128, 512, None, 0, 0)),
    (('fwd', 16, 384, 0, 32, 32, 512, 3, 1, 'bn'), ('conv_halo_k32_kernel<8,128>', 1128, 64, None, 1, 1)),
    (('dgrad', 16, 384, 0, 32, 32, 512, 3, 1, ''), ('conv_halo_k32_kernel<8,128>', 1128, 64, None, 1, 1)),
    (('fwd', 16, 256, 0, 64, 64, 384, 1, 1, 'bn'), ('conv_igemm_dma_x3_kernel<128>', 128, 512, None, 0, 0)),
    (('fwd', 16, 3, 0, 128, 128, 256, 3, 1, 'bn'), ('thin32_cin_kernel', 0, 0, 0, 0, 0)),
    (('dgrad', 16, 3, 0, 128, 128, 256, 3, 1, ''), ('thin32_cin_kernel', 0, 0, 0, 0, 0)),
    (('fwd', 16, 8, 0, 256, 256, 3, 3, 1, 'bn'), ('conv_igemm_kernel<256,32>', 0, 0, 0, 0, 0)),
    (('dgrad', 16, 8, 0, 256, 256, 3, 3, 1, ''), ('conv_igemm_kernel<256,32>', 0, 0, 0, 0, 0)),
    (('fwd', 16, 128, 0, 128, 128, 256, 1, 1, 'bn'), ('conv_igemm_dma_x3_kernel<128>', 128, 2048, None, 0, 0)),
    (('wgrad', 16, 3, 0, 256, 256, 8, 3, 1, ''), ('wgrad_tiny4_kernel', 294912, None)),
    (('fwd', 16, 128, 0, 256, 256, 64, 1, 1, 'bn'), ('conv_igemm_dma_x3_kernel<64>', 64, 8192, None, 0, 0)),
    (('fwd', 16, 384, 0, 64, 64, 256, 1, 1, 'bn'), ('conv_igemm_dma_x3_kernel<128>', 128, 512, None, 0, 0)),
    (('wgrad', 16, 128, 0, 128, 128, 256, 1, 1, ''), ('wgrad_dma_x3_kernel<128,128>', 67108864, None)),
    (('fwd', 16, 256, 0, 128, 128, 128, 1, 1, 'bn'), ('conv_igemm_dma_x3_kernel<128>', 128, 2048, None, 0, 0)),
    (('wgrad', 16, 32, 0, 32, 32, 1024, 3, 1, ''), ('wgrad_halo_x3_kernel<32,128>', 75497472, None)),
    (('wgrad', 16, 1024, 0, 32, 32, 512, 1, 1, ''), ('wgrad_dma_x3_kernel<128,128>', 67108864, None)),
    (('wgrad', 16, 384, 0, 64, 64, 256, 1, 1, ''), ('wgrad_dma_x3_kernel<128,128>', 64487424, None)),
    (('wgrad', 16, 256, 0, 64, 64, 384, 1, 1, ''), ('wgrad_dma_x3_kernel<128,128>', 64487424, None)),
    (('fwd', 16, 768, 0, 16, 16, 512, 1, 1, 'bn'), ('conv_igemm_dma_x3_kernel<128>', 128, 32, None, 0, 0)),
    (('fwd', 16, 3, 0, 512, 512, 4, 3, 1, 'bn'), ('tiny4_kernel', 0, 0, 0, 0, 0)),
    (('dgrad', 16, 3, 0, 512, 512, 4, 3, 1, ''), ('tiny4_kernel', 0, 0, 0, 0, 0)),
    (('fwd', 16, 3, 0, 64, 64, 384, 3, 1, 'bn'), ('thin32_cin_kernel', 0, 0, 0, 0, 0)),
    (('dgrad', 16, 3, 0, 64, 64, 384, 3, 1, ''), ('thin32_cin_kernel', 0, 0, 0, 0, 0)),
    (('fwd', 16, 512, 0, 32, 32, 512, 1, 1, 'bn'), ('conv_igemm_dma_x3_kernel<128>', 128, 128, None, 0, 0)),
    (('wgrad', 16, 384, 0, 64, 64, 3, 3, 1, ''), ('wgrad4_kernel<thin_cout>', 10616832, None)),
    (('fwd', 16, 32, 0, 32, 32, 1024, 3, 1, 'bn'), ('conv_halo_k32_kernel<8,128>', 1128, 64, None, 1, 1)),
    (('dgrad', 16, 32, 0, 32, 32, 1024, 3, 1, ''), ('conv_halo_k32_kernel<8,128>', 1128, 64, None, 1, 1)),
    (('fwd', 16, 384, 0, 64, 64, 3, 3, 1, 'bn'), ('thin4_cout_kernel', 0, 0, 0, 0, 0)),
    (('dgrad', 16, 384, 0, 64, 64, 3, 3, 1, ''), ('thin4_cout_kernel', 0, 0, 0, 0, 0)),
    (('fwd', 16, 512, 0, 32, 32, 384, 1, 1, 'bn'), ('conv_igemm_dma_x3_kernel<128>', 128, 128, None, 0, 0)),
    (('fwd', 16, 4, 0, 512, 512, 3, 3, 1, 'bn'), ('tiny4_kernel', 0, 0, 0, 0, 0)),
    (('dgrad', 16, 4, 0, 512, 512, 3, 3, 1, ''), ('tiny4_kernel', 0, 0, 0, 0, 0)),
    (('fwd', 16, 16, 0, 128, 128, 3, 3, 1, 'bn'), ('thin_small_cout_kernel', 0, 0, 0, 0, 0)),
    (('dgrad', 16, 16, 0, 128, 128, 3, 3, 1, ''), ('thin_small_cout_kernel', 0, 0, 0, 0, 0)),
    (('fwd', 16, 384, 0, 32, 32, 512, 1, 1, 'bn'), ('conv_igemm_dma_x3_kernel<128>', 128, 128, None, 0, 0)),
    (('fwd', 16, 1024, 0, 32, 32, 512, 1, 1, 'bn'), ('conv_igemm_dma_x3_kernel<128>', 128, 128, None, 0, 0)),
    (('fwd', 16, 512, 0, 16, 16, 768, 1, 1, 'bn'), ('conv_igemm_dma_x3_kernel<128>', 128, 32, None, 0, 0)),
    (('wgrad', 16, 3, 0, 128, 128, 16, 3, 1, ''), ('wgrad4_kernel<thin_cin>', 4718592, None)),
    (('fwd', 16, 3, 0, 256, 256, 8, 3, 1, 'bn'), ('tiny4_kernel', 0, 0, 0, 0, 0)),
    (('dgrad', 16, 3, 0, 256, 256, 8, 3, 1, ''), ('tiny4_kernel', 0, 0, 0, 0, 0)),
    (('fwd', 16, 512, 0, 32, 32, 3, 3, 1, 'bn'), ('thin4_cout_kernel', 0, 0, 0, 0, 0)),
    (('dgrad', 16, 512, 0, 32, 32, 3, 3, 1, ''), ('thin4_cout_kernel', 0, 0, 0, 0, 0)),
    (('fwd', 16, 1536, 0, 16, 16, 48, 3, 1, 'bn'), ('conv_igemm_halo16_kernel<128,64>+splitk', 0, 0, 12582912, 0, 0)),
    (('dgrad', 16, 1536, 0, 16, 16, 48, 3, 1, ''), ('conv_igemm_halo16_kernel<128,64>+splitk', 0, 0, 12582912, 0, 0)),
    (('fwd', 16, 48, 0, 16, 16, 1536, 3, 1, 'bn'), ('conv_igemm_halo16_kernel<128,128>', 0, 32, None, 0, 0)),
    (('dgrad', 16, 48, 0, 16, 16, 1536, 3, 1, ''), ('conv_igemm_halo16_kernel<128,128>', 0, 32, 0, 0, 0)),
    (('wgrad', 16, 512, 0, 32, 32, 384, 1, 1, ''), ('wgrad_dma_x3_kernel<128,128>', 50331648, None)),
    (('wgrad', 16, 48, 0, 16, 16, 1536, 3, 1, ''), ('wgrad_dma_x3_kernel<128,128>', 42467328, None)),
    (('wgrad', 16, 384, 0, 32, 32, 512, 1, 1, ''), ('wgrad_dma_x3_kernel<128,128>', 50331648, None)),
    (('wgrad', 16, 512, 0, 32, 32, 3, 3, 1, ''), ('wgrad4_kernel<thin_cout>', 7077888, None)),
    (('fwd', 16, 3, 0, 32, 32, 512, 3, 1, 'bn'), ('thin4_cin_kernel', 0, 0, 0, 0, 0)),
    (('dgrad', 16, 3, 0, 32, 32, 512, 3, 1, ''), ('thin4_cin_kernel', 0, 0, 0, 0, 0)),
    (('fwd', 16, 3, 0, 128, 128, 16, 3, 1, 'bn'), ('thin4_cin_kernel', 0, 0, 0, 0, 0)),
    (('dgrad', 16, 3, 0, 128, 128, 16, 3, 1, ''), ('thin4_cin_kernel', 0, 0, 0, 0, 0)),
    (('fwd', 16, 24, 0, 64, 64, 3, 3, 1, 'bn'), ('thin_small_cout_kernel', 0, 0, 0, 0, 0)),
    (('dgrad', 16, 24, 0, 64, 64, 3, 3, 1, ''), ('thin_small_cout_kernel', 0, 0, 0, 0, 0)),
    (('fwd', 16, 32, 0, 32, 32, 3, 3, 1, 'bn'), ('thin_small_cout_kernel', 0, 0, 0, 0, 0)),
    (('dgrad', 16, 32, 0, 32, 32, 3, 3, 1, ''), ('thin_small_cout_kernel', 0, 0, 0, 0, 0)),
    (('wgrad', 16, 768, 0, 16, 16, 512, 1, 1, ''), ('wgrad_dma_x3_kernel<128,128>', 25165824, None)),
    (('wgrad', 16, 512, 0, 16, 16, 768, 1, 1, ''), ('wgrad_dma_x3_kernel<128,128>', 25165824, None)),
    (('fwd', 16, 768, 0, 16, 16, 3, 3, 1, 'bn'), ('thin4_cout_kernel', 0, 0, 0, 0, 0)),
    (('dgrad', 16, 768, 0, 16, 16, 3, 3, 1, ''), ('thin4_cout_kernel', 0, 0, 0, 0, 0)),
    (('wgrad', 16, 3, 0, 64, 64, 24, 3, 1, ''), ('wgrad4_kernel<thin_cin>', 1769472, None)),
    (('wgrad', 16, 3, 0, 32, 32, 32, 3, 1, ''), ('wgrad4_kernel<thin_cin>', 589824, None)),
    (('fwd', 16, 3, 0, 64, 64, 24, 3, 1, 'bn'), ('thin4_cin_kernel', 0, 0, 0, 0, 0)),
    (('dgrad', 16, 3, 0, 64, 64, 24, 3, 1, ''), ('thin4_cin_kernel', 0, 0, 0, 0, 0)),
    (('fwd', 16, 3, 0, 32, 32, 32, 3, 1, 'bn'), ('thin4_cin_kernel', 0, 0, 0, 0, 0)),
    (('dgrad', 16, 3, 0, 32, 32, 32, 3, 1, ''), ('thin4_cin_kernel', 0, 0, 0, 0, 0)),
    (('fwd', 16, 48, 0, 16, 16, 3, 3, 1, 'bn'), ('thin_small_cout_kernel', 0, 0, 0, 0, 0)),
    (('dgrad', 16, 48, 0, 16, 16, 3, 3, 1, ''), ('thin_small_cout_kernel', 0, 0, 0, 0, 0)),
    (('fwd', 1, 1, 0, 1, 16, 1024, 1, 1, 'bn'), ('thin4_cin_kernel', 0, 0, 0, 0, 0)),
    (('fwd', 16, 3, 0, 16, 16, 768, 3, 1, 'bn'), ('thin4_cin_kernel', 0, 0, 0, 0, 0)),
    (('dgrad', 16, 3, 0, 16, 16, 768, 3, 1, ''), ('thin4_cin_kernel', 0, 0, 0, 0, 0)),
    (('wgrad', 16, 768, 0, 16, 16, 3, 3, 1, ''), ('wgrad4_kernel<thin_cout>', 5308416, None)),
    (('fwd', 16, 3, 0, 16, 16, 48, 3, 1, 'bn'), ('thin4_cin_kernel', 0, 0, 0, 0, 0)),
    (('dgrad', 16, 3, 0, 16, 16, 48, 3, 1, ''), ('thin4_cin_kernel', 0, 0, 0, 0, 0)),
    (('wgrad', 16, 3, 0, 16, 16, 48, 3, 1, ''), ('wgrad4_kernel<thin_cin>', 442368, None)),
    (('fwd', 16, 768, 0, 16, 16, 768, 3, 1, ''), ('conv_igemm_halo16_kernel<128,128>+splitk', 0, 0, 50331648, 0, 0)),
    (('fwd', 16, 1024, 0, 32, 32, 32, 3, 1, ''), ('conv_igemm_halo_kernel<128,64>+splitk', 0, 0, 12582912, 0, 0)),
    (('fwd', 16, 512, 0, 32, 32, 128, 3, 1, ''), ('conv_igemm_halo_kernel<128,64>+splitk', 0, 0, 25165824, 0, 0)),
    (('fwd', 4, 512, 0, 32, 32, 128, 3, 1, 'bn'), ('conv_igemm_halo_kernel<128,64>+splitk', 0, 0, 16777216, 0, 0)),
    (('fwd', 4, 512, 0, 32, 32, 128, 3, 1, 'fp32'), ('conv_igemm_halo_kernel<128,64>+splitk', 0, 0, 16777216, 0, 0)),
    (('fwd', 4, 512, 0, 32, 32, 128, 3, 1, 'k32=2'), ('conv_halo_k32_kernel<8,128>', 1128, 16, None, 1, 1)),
    (('fwd', 2, 256, 0, 64, 64, 64, 3, 1, ''), ('conv_igemm_halo_kernel<128,64>+splitk', 0, 0, 8388608, 0, 0)),
    (('fwd', 2, 256, 0, 64, 64, 64, 3, 1, 'k32=2'), ('conv_halo_k32_kernel<16,64>', 1064, 16, None, 0, 1)),
    (('fwd', 16, 1536, 0, 16, 16, 48, 3, 1, ''), ('conv_igemm_halo16_kernel<128,64>+splitk', 0, 0, 12582912, 0, 0)),
    (('fwd', 16, 512, 0, 128, 128, 16, 3, 1, ''), ('conv_halo_k32_kernel<8,16>', 1016, 1024, None, 0, 0)),
    (('fwd', 16, 512, 0, 128, 128, 16, 3, 1, 'k32=0'), ('conv_igemm_kernel<256,32>', 0, 0, 0, 0, 0)),
    (('fwd', 16, 512, 0, 128, 128, 16, 3, 1, 'fp32'), ('conv_igemm_kernel<256,32>', 0, 0, 0, 0, 0)),
    (('fwd', 2, 512, 0, 64, 64, 32, 3, 1, ''), ('conv_igemm_halo_kernel<128,64>+splitk', 0, 0, 8388608, 0, 0)),
    (('fwd', 2, 512, 0, 64, 64, 32, 3, 1, 'k32=2'), ('conv_halo_k32_kernel<8,32>', 1032, 32, None, 0, 0)),
    (('fwd', 16, 64, 0, 128, 128, 16, 3, 1, ''), ('conv_igemm_kernel<256,32>', 0, 0, 0, 0, 0)),
    (('fwd', 16, 128, 0, 128, 128, 20, 3, 1, ''), ('conv_halo_k32_kernel<8,32>', 1032, 1024, None, 0, 0)),
    (('fwd', 16, 128, 0, 128, 128, 8, 3, 1, 'k32=2'), ('thin4_cout_kernel', 0, 0, 0, 0, 0)),
    (('dgrad', 2, 64, 0, 32, 32, 64, 3, 2, 'parity'), ('declined', 0, 2, 0, 0, 0)),
    (('dgrad', 2, 64, 0, 34, 34, 64, 3, 2, 'parity'), ('conv_igemm_halo_x3_kernel<128,64,4,1,true>', 64, 12, None, 0, 0)),
    (('dgrad', 2, 64, 0, 64, 64, 96, 3, 2, 'parity'), ('declined', 0, 16, 0, 0, 0)),
    (('dgrad', 16, 64, 0, 512, 512, 64, 3, 2, 'parity fp32'), ('declined', 0, 4096, 0, 0, 0)),
    (('dgrad', 2, 64, 0, 32, 32, 64, 3, 2, 'class=0'), ('conv_igemm_dma_kernel<128,64>', 0, 4, 0, 0, 0)),
    (('dgrad', 2, 64, 0, 32, 32, 64, 3, 2, 'class=1'), ('conv_igemm_dma_kernel<128,64>', 0, 4, 0, 0, 0)),
    (('dgrad', 2, 64, 0, 32, 32, 64, 3, 2, 'class=2'), ('conv_igemm_dma_kernel<128,64>', 0, 4, 0, 0, 0)),
    (('dgrad', 2, 64, 0, 32, 32, 64, 3, 2, 'class=3'), ('conv_igemm_dma_kernel<128,64>', 0, 4, 0, 0, 0)),
    (('dgrad', 16, 64, 0, 512, 512, 64, 3, 2, 'class=3'), ('conv_igemm_dma_x3_kernel<64>', 64, 8192, None, 0, 0)),
    (('dgrad', 16, 64, 0, 512, 512, 64, 3, 2, 'class=0 fp32'), ('conv_igemm_dma_kernel<128,64>', 0, 8192, 0, 0, 0)),
    (('fwd', 16, 3, 0, 512, 512, 64, 3, 1, 'bias'), ('thin32_cin_kernel', 0, 0, 0, 0, 0)),
    (('fwd', 16, 4, 0, 512, 512, 4, 3, 1, ''), ('tiny4_kernel', 0, 0, 0, 0, 0)),
    (('fwd', 16, 64, 0, 512, 512, 3, 1, 1, ''), ('thin4_cout_kernel', 0, 0, 0, 0, 0)),
    (('fwd', 16, 64, 0, 512, 512, 128, 1, 1, ''), ('conv1x1_k64_kernel', 0, 32768, 0, 0, 0)),
    (('fwd', 16, 64, 0, 512, 512, 128, 1, 1, 'fp32 bn'), ('conv_igemm_dma_kernel<128,64>', 0, 32768, None, 0, 0)),
    (('fwd', 16, 64, 0, 256, 256, 64, 1, 1, 'res relu'), ('conv1x1_k64_kernel', 0, 8192, 0, 0, 0)),
    (('fwd', 1, 1024, 0, 1, 16, 18432, 1, 1, 'bias'), ('conv_igemm_dma_kernel<128,128>', 0, 1, 0, 0, 0)),
    (('fwd', 2, 8, 0, 64, 64, 3, 3, 1, ''), ('conv_igemm_kernel<256,32>', 0, 0, 0, 0, 0)),
    (('fwd', 16, 64, 64, 256, 256, 64, 3, 1, 'bn'), ('conv_halo_k32_kernel<16,64>', 1064, 2048, None, 0, 1)),
    (('fwd', 16, 128, 64, 128, 128, 128, 3, 1, 'bn'), ('conv_halo_k32_kernel<8,128>', 1128, 1024, None, 0, 1)),
    (('fwd', 16, 64, 16, 256, 256, 64, 3, 1, 'bn'), ('conv_igemm_halo_x3_kernel<128,64>', 64, 8192, None, 0, 0)),
    (('fwd', 16, 128, 128, 128, 128, 128, 1, 1, ''), ('conv_igemm_dma_x3_kernel<128>', 128, 2048, None, 0, 0)),
    (('fwd', 4, 512, 256, 32, 32, 256, 3, 1, ''), ('conv_igemm_halo_kernel<128,64>+splitk', 0, 0, 25165824, 0, 0)),
    (('fwd', 16, 64, 0, 512, 512, 64, 3, 1, 'mis'), ('conv_igemm_halo_x3_kernel<128,64>', 64, 32768, None, 0, 0)),
    (('fwd', 16, 64, 0, 512, 512, 64, 3, 1, 'mis bn'), ('conv_igemm_halo_x3_kernel<128,64>', 64, 32768, None, 0, 0)),
    (('fwd', 16, 512, 0, 32, 32, 128, 3, 1, 'mis'), ('conv_igemm_halo_x3_kernel<128,64>', 64, 128, None, 0, 0)),
    (('fwd', 16, 512, 0, 128, 128, 16, 3, 1, 'mis'), ('conv_igemm_kernel<256,32>', 0, 0, 0, 0, 0)),
    (('fwd', 16, 128, 0, 256, 256, 128, 1, 1, 'mis'), ('conv_igemm_dma_x3_kernel<128>', 128, 8192, None, 0, 0)),
    (('fwd', 16, 128, 0, 256, 256, 128, 3, 1, 'bias relu'), ('conv_halo_k32_kernel<8,128>', 1128, 4096, None, 1, 0)),
    (('fwd', 16, 64, 0, 512, 512, 64, 3, 1, 'res'), ('conv_halo_k32_kernel<16,64>', 1064, 8192, None, 0, 0)),
    (('fwd', 16, 64, 0, 512, 512, 64, 3, 1, 'aff bn'), ('conv_halo_k32_kernel<4,64>', 1064, 32768, None, 1, 0)),
    (('fwd', 16, 128, 0, 256, 256, 128, 3, 1, 'aff bn'), ('conv_halo_k32_kernel<8,128>', 1128, 4096, None, 1, 0)),
    (('fwd', 16, 64, 0, 512, 512, 64, 3, 1, 'aff fp32'), ('declined', 0, 32768, 0, 0, 0)),
    (('fwd', 16, 128, 0, 256, 256, 128, 1, 1, 'aff'), ('declined', 128, 8192, None, 0, 0)),
    (('fwd', 16, 64, 64, 256, 256, 64, 3, 1, 'aff'), ('declined', 1064, 8192, None, 0, 0)),
    (('fwd', 4, 512, 0, 32, 32, 128, 3, 1, 'aff'), ('declined', 0, 0, 16777216, 0, 0)),
    (('fwd', 4, 512, 0, 32, 32, 128, 3, 1, 'aff k32=2'), ('conv_halo_k32_kernel<8,128>', 1128, 16, None, 1, 0)),
    (('fwd', 16, 128, 0, 256, 256, 128, 3, 1, 'aff k32=0'), ('declined', 128, 8192, None, 0, 0)),
    (('dgrad', 16, 64, 0, 512, 512, 64, 3, 1, 'bwd'), ('conv_halo_k32_kernel<16,64>', 1064, 8192, None, 0, 1)),
    (('dgrad', 16, 128, 0, 256, 256, 128, 3, 1, 'bwd'), ('conv_halo_k32_kernel<8,128>', 1128, 4096, None, 1, 1)),
    (('dgrad', 16, 128, 0, 128, 128, 64, 3, 1, 'bwd'), ('conv_halo_k32_kernel<4,64>', 1064, 2048, None, 1, 1)),
    (('dgrad', 16, 64, 0, 512, 512, 64, 3, 1, 'bwd res'), ('declined', 1064, 8192, None, 0, 0)),
    (('dgrad', 16, 64, 0, 512, 512, 64, 3, 1, 'bwd fp32'), ('declined', 0, 32768, 0, 0, 0)),
    (('dgrad', 4, 512, 0, 32, 32, 128, 3, 1, 'bwd'), ('declined', 0, 0, 16777216, 0, 0)),
    (('dgrad', 16, 128, 0, 256, 256, 128, 3, 1, 'bwd k32=0'), ('declined', 128, 8192, None, 0, 0)),
    (('fwd', 16, 64, 0, 512, 512, 64, 3, 1, 'fp32 bn'), ('conv_igemm_halo_kernel<128,64>', 0, 32768, None, 0, 0)),
    (('fwd', 16, 128, 0, 256, 256, 128, 3, 1, 'fp32 bn'), ('conv_igemm_halo_kernel<128,128>', 0, 8192, None, 0, 0)),
    (('fwd', 16, 64, 0, 256, 256, 64, 3, 2, 'fp32 bn'), ('conv_igemm_dma_kernel<256,64>', 0, 1024, None, 0, 0)),
    (('fwd', 16, 128, 0, 256, 256, 256, 1, 1, 'fp32'), ('conv_igemm_dma_kernel<128,64>', 0, 8192, 0, 0, 0)),
    (('fwd', 16, 512, 0, 32, 32, 512, 3, 1, 'fp32 bn'), ('conv_igemm_halo_kernel<128,64>', 0, 128, None, 0, 0)),
    (('fwd', 16, 768, 0, 16, 16, 768, 3, 1, 'fp32'), ('conv_igemm_halo16_kernel<128,128>+splitk', 0, 0, 50331648, 0, 0)),
    (('dgrad', 16, 64, 0, 256, 256, 128, 3, 1, 'fp32'), ('conv_igemm_halo_kernel<128,128>', 0, 8192, 0, 0, 0)),
    (('fwd', 16, 64, 0, 512, 512, 64, 3, 1, 'bn k32=0'), ('conv_igemm_halo_x3_kernel<128,64>', 64, 32768, None, 0, 0)),
    (('fwd', 16, 64, 0, 512, 512, 64, 3, 1, 'bn k32=1'), ('conv_halo_k32_kernel<16,64>', 1064, 8192, None, 0, 1)),
    (('fwd', 16, 64, 0, 512, 512, 64, 3, 1, 'bn k32=2'), ('conv_halo_k32_kernel<16,64>', 1064, 8192, None, 0, 1)),
    (('fwd', 16, 128, 0, 256, 256, 128, 3, 1, 'bn k32=0'), ('conv_igemm_halo_x3_kernel<128,128>', 128, 8192, None, 0, 0)),
    (('fwd', 16, 128, 0, 256, 256, 128, 3, 1, 'bn k32=1'), ('conv_halo_k32_kernel<8,128>', 1128, 4096, None, 1, 1)),
    (('fwd', 16, 128, 0, 256, 256, 128, 3, 1, 'bn k32=2'), ('conv_halo_k32_kernel<8,128>', 1128, 4096, None, 1, 1)),
    (('fwd', 16, 256, 0, 64, 64, 256, 3, 1, 'k32=0'), ('conv_igemm_halo_x3_kernel<128,128>', 128, 512, None, 0, 0)),
    (('fwd', 16, 256, 0, 64, 64, 256, 3, 1, 'k32=1'), ('conv_halo_k32_kernel<8,128>', 1128, 256, None, 1, 1)),
    (('fwd', 16, 256, 0, 64, 64, 256, 3, 1, 'k32=2'), ('conv_halo_k32_kernel<8,128>', 1128, 256, None, 1, 1)),
    (('fwd', 16, 512, 0, 32, 32, 512, 3, 1, 'bn k32=0'), ('conv_igemm_halo_x3_kernel<128,64>', 64, 128, None, 0, 0)),
    (('fwd', 16, 512, 0, 32, 32, 512, 3, 1, 'bn k32=1'), ('conv_halo_k32_kernel<8,128>', 1128, 64, None, 1, 1)),
    (('fwd', 16, 512, 0, 32, 32, 512, 3, 1, 'bn k32=2'), ('conv_halo_k32_kernel<8,128>', 1128, 64, None, 1, 1)),
    (('fwd', 16, 768, 0, 64, 64, 24, 3, 1, 'k32=0'), ('conv_igemm_kernel<256,32>', 0, 0, 0, 0, 0)),
    (('fwd', 16, 768, 0, 64, 64, 24, 3, 1, 'k32=1'), ('conv_halo_k32_kernel<8,32>', 1032, 256, None, 0, 0)),
    (('fwd', 16, 768, 0, 64, 64, 24, 3, 1, 'k32=2'), ('conv_halo_k32_kernel<8,32>', 1032, 256, None, 0, 0)),
    (('fwd', 16, 64, 0, 256, 256, 64, 3, 2, 'bn k32=0'), ('conv_igemm_dma_x3_kernel<64>', 64, 2048, None, 0, 0)),
    (('fwd', 16, 64, 0, 256, 256, 64, 3, 2, 'bn k32=1'), ('conv_igemm_dma_x3_kernel<64>', 64, 2048, None, 0, 0)),
    (('fwd', 16, 64, 0, 256, 256, 64, 3, 2, 'bn k32=2'), ('conv_igemm_dma_x3_kernel<64>', 64, 2048, None, 0, 0)),
    (('dgrad', 16, 128, 0, 256, 256, 64, 3, 1, 'k32=0'), ('conv_igemm_halo_x3_kernel<128,64>', 64, 8192, None, 0, 0)),
    (('dgrad', 16, 128, 0, 256, 256, 64, 3, 1, 'k32=1'), ('conv_halo_k32_kernel<16,64>', 1064, 2048, None, 0, 1)),
    (('dgrad', 16, 128, 0, 256, 256, 64, 3, 1, 'k32=2'), ('conv_halo_k32_kernel<16,64>', 1064, 2048, None, 0, 1)),
    (('fwd', 2, 64, 0, 48, 48, 64, 3, 1, 'k32=0'), ('conv_igemm_halo_x3_kernel<128,64>', 64, 48, None, 0, 0)),
    (('fwd', 2, 64, 0, 48, 48, 64, 3, 1, 'k32=1'), ('conv_igemm_halo_x3_kernel<128,64>', 64, 48, None, 0, 0)),
    (('fwd', 2, 64, 0, 48, 48, 64, 3, 1, 'k32=2'), ('conv_halo_k32_kernel<16,64>', 1064, 12, None, 0, 1)),
    (('wgrad', 16, 64, 0, 512, 512, 64, 3, 1, 'wk32=0'), ('wgrad_halo_x3_kernel<64,64>', 75497472, None)),
    (('wgrad', 16, 64, 0, 512, 512, 64, 3, 1, 'wk32=1'), ('wgrad_k32_kernel<64,64>', 150994944, None)),
    (('wgrad', 16, 128, 0, 256, 256, 128, 3, 1, 'wk32=0'), ('wgrad_halo_x3_kernel<32,128>', 150994944, None)),
    (('wgrad', 16, 128, 0, 256, 256, 128, 3, 1, 'wk32=1'), ('wgrad_k32_kernel<64,64>', 150994944, None)),
    (('wgrad', 16, 768, 0, 16, 16, 768, 3, 1, 'wk32=0'), ('wgrad_halo_x3_kernel<32,128>', 148635648, None)),
    (('wgrad', 16, 768, 0, 16, 16, 768, 3, 1, 'wk32=1'), ('wgrad_halo_x3_kernel<32,128>', 148635648, None)),
    (('wgrad', 16, 512, 0, 32, 32, 512, 3, 1, 'wk32=0'), ('wgrad_halo_x3_kernel<32,128>', 150994944, None)),
    (('wgrad', 16, 512, 0, 32, 32, 512, 3, 1, 'wk32=1'), ('wgrad_k32_kernel<64,64>', 150994944, None)),
    (('wgrad', 2, 64, 0, 64, 64, 64, 3, 1, 'wk32=0'), ('wgrad_halo_x3_kernel<64,64>', 4718592, None)),
    (('wgrad', 2, 64, 0, 64, 64, 64, 3, 1, 'wk32=1'), ('wgrad_k32_kernel<64,64>', 4718592, None)),
    (('wgrad', 16, 64, 0, 512, 512, 64, 3, 1, 'fp32'), ('wgrad_halo_kernel<64,64>', 75497472, None)),
    (('wgrad', 16, 128, 0, 256, 256, 128, 3, 1, 'fp32'), ('wgrad_halo_kernel<32,128>', 150994944, None)),
    (('wgrad', 16, 64, 0, 512, 512, 64, 3, 2, 'fp32'), ('wgrad_dma_kernel<128,64>', 30081024, None)),
    (('wgrad', 16, 768, 0, 16, 16, 768, 3, 1, 'fp32'), ('wgrad_halo_kernel<32,128>', 148635648, None)),
    (('wgrad', 16, 64, 0, 256, 256, 128, 1, 1, 'fp32'), ('wgrad_dma_kernel<128,128>', 16777216, None)),
    (('wgrad', 16, 16, 0, 128, 128, 16, 3, 1, ''), ('wgrad_kernel<128,32>', 4718592, None)),
    (('wgrad', 16, 64, 0, 512, 512, 64, 3, 1, 'aff'), ('wgrad_k32_kernel<64,64>', 150994944, 1)),
    (('wgrad', 16, 128, 0, 256, 256, 128, 3, 1, 'aff'), ('wgrad_k32_kernel<64,64>', 150994944, 1)),
    (('wgrad', 16, 64, 0, 512, 512, 64, 3, 2, 'aff'), ('declined', None, 0)),
    (('wgrad', 16, 64, 64, 256, 256, 64, 3, 1, 'aff'), ('declined', None, 0)),
    (('wgrad', 16, 64, 64, 256, 256, 64, 3, 1, ''), ('wgrad_k32_kernel<64,64>', 150994944, None)),
    (('wgrad', 16, 64, 0, 512, 512, 3, 3, 1, 'aff'), ('declined', None, 0)),
    (('wgrad', 16, 128, 0, 256, 256, 128, 3, 1, 'aff wk32=0'), ('declined', None, 0)),
    (('wgrad', 16, 3, 0, 512, 512, 64, 3, 1, 'fp32'), ('wgrad32_cin_kernel', 18874368, None)),
    (('wgrad', 2, 8, 0, 64, 64, 3, 3, 1, ''), ('wgrad_kernel<128,32>', 27648, None)),
]


@pytest.mark.parametrize('spec,want', ROWS, ids=['%s n%d c%d+%d %dx%d o%d k%d s%d %s' % s[:10] for s, _ in ROWS])
def test_launch_plan(pkg, spec, want):
    assert run_row(pkg._lib, pkg.ops._CONV_LABELS, pkg.ops._WGRAD_LABELS, spec) == want
