"""Plain references for ssg_conv2d_f32 / ssg_conv2d_igemm_f32 (csrc/conv_igemm*.hip, conv_thin*.hip, conv_1x1.hip): the dense
convolution's forward and input gradient on every kernel route, and for the weight packs they read.  Plain helper module in the
style of wgrad_ref.py (not a conftest, no fixtures), numpy only; nothing here calls an op under test.

* case       -- one ssg_conv_desc launch described at descriptor level, with THE KERNEL ID IT EXPECTS AS A LITERAL (and the pack
                format, split-K slab count and LDS-DMA body it expects): plan_conv is not restated here (tests/test_conv_plan.py
                pins its decisions); tests/test_conv_ref.py and tests/test_conv_gpu.py check the literals against the library;
* conv_ref   -- the launch in fp64, written from the contract in the header comment of ssg_conv_desc (include/ssunet_hip.h), with
                its magnitude sum and the fp64 statistics rows;
* packs      -- ssg_pack_weights_f32 (kmode 0 / 1, transpose, tap order, Cred_pad, zero padding to Kp) and the 64 / 128 and
                1016 / 1032 / 1064 / 1128 layouts of ssg_pack_weights_split_bf16x3, restated;
* data       -- three classes as in wgrad_ref: (a) integer-valued operands (exact), (b) one non-zero input pixel and channel
                (every output element one product), (c) random full-mantissa operands with non-zero means;
* gates      -- derived beside each; none is measured;
* case table -- the smallest shapes at which each route can still go wrong, and check_coverage();
* emul       -- the launch in numpy float32, one K-step at a time in the route's K order (six bf16-term products, small ones
                first, on split routes; slabs in order for split-K), with the planted defects of tests/test_conv_ref.py as
                keyword switches (all off).

Kernel ids (ssg_conv2d_kernel_id), all reachable on this entry point: 0 / 1 / 2 conv_igemm_kernel<128,128> / <256,64> / <256,32>
(register-staged: kmode 1, or Cout <= 32); 10 thin small-Cout (VALU); 12 / 13 thin4 (4x4x1 MFMA: 4-channel input / Cout <= 8 with
C1 % 64 == 0); 14 tiny4; 15 thin32; 16 conv1x1_k64; 20 / 21 / 22 conv_igemm_dma_kernel; 30 / 31 / 32 conv_igemm_halo_kernel;
33 / 34 conv_igemm_halo16_kernel; 40 / 41 conv_igemm_halo_x3_kernel; 42 the merged parity classes; 50 / 51 conv_igemm_dma_x3 (two
bodies: ssg_conv_dma_body 1 = conv_igemm_dma_x3_kernel, 2 = the split-once body of conv_igemm_dma_k32.hip); 60..64
conv_halo_k32_kernel<8,128> / <4,64> / <16,64> / <8,16> / <8,32>.  UNREACHABLE_IDS is empty: unlike the weight gradient, kmode 1
keeps Cout > 32 on the register-staged kernels (ids 0 and 1), and thin4 kinds 3 and 4 give ids 12 and 13.

No case is filtered by value and no gate holds a measured number."""
from collections import namedtuple

import numpy as np

from bn_ref import ACT_LRELU, ACT_NONE, ACT_RELU, F32, F64, U32, cdiv, f32, preact_emul, same_bits, worst_ratio  # noqa: F401
from wgrad_ref import (C_SPLIT, FLT_MAX, LRELU_SLOPE, RMS_MARGIN, _full, _pow2, act32, classes, pad4, product_gate, rms,  # noqa: F401
                       split3)

REACHABLE_IDS = (0, 1, 2, 10, 12, 13, 14, 15, 16, 20, 21, 22, 30, 31, 32, 33, 34, 40, 41, 42, 50, 51, 60, 61, 62, 63, 64)
UNREACHABLE_IDS = ()
SPLIT_IDS = (40, 41, 42, 50, 51, 60, 61, 62, 63, 64)     # both operands as three bf16 terms, six products (mfma_split.h)
K32_IDS = (60, 61, 62, 63, 64)                           # K-step = one tap x 32 channels; every other kmode-0 route: one tap x 16
# pixel tile (th, tw) of the statistics epilogue: one bnpart row per tile, ssg_conv2d_bnpart_rows = N ceil(GH / th) ceil(GW / tw)
STAT_TILE = {20: (8, 16), 21: (16, 16), 22: (8, 16), 30: (4, 32), 31: (8, 32), 32: (4, 32), 33: (8, 16), 34: (8, 16), 40: (4, 32),
             41: (4, 32), 50: (8, 16), 51: (8, 16), 60: (8, 32), 61: (4, 32), 62: (16, 32), 63: (8, 32), 64: (8, 32)}
# pixel tile and column tile of every route that has one (the ragged-tile facts of check_coverage)
OUT_TILE = dict(list(STAT_TILE.items()) + [(0, (8, 16)), (1, (16, 16)), (2, (16, 16)), (42, (4, 32))])
COL_TILE = {0: 128, 1: 64, 2: 32, 20: 128, 21: 64, 22: 64, 30: 128, 31: 64, 32: 64, 33: 128, 34: 64}


# ============================================================================ 1. the case type and its geometry
# op 'fwd': x [N, H, W, C1 | C2] -> y [N, oh, ow, Cout], weights OIHW [Cout, cred_real, k, k].
# op 'dgrad': dy [N, oh, ow, C1] -> dx [N, H, W, Cout] = input channels [c_lo, c_lo + Cout) of the ctot the forward conv has; weights
#   OIHW [cred_real, ctot, k, k], packed transposed, desc.w offset by c_lo rows; cls: None (stride 1, taps mirrored), 'merge'
#   (parity_merge = 1) or (py, px) (one parity class of stride 2).
# H x W is the FORWARD conv's input in both ops (the convention of tests/test_conv_plan.py); pad = k // 2.
# cred_real: reduced channels that are real (None = C1 + C2): the rest are pad channels with zero weights (Cred_pad of the pack).
# bias / res: bool; act: epilogue activation; ld*: None = dense (pad4); split: w_split given where ssg_conv2d_split_bn != 0
# (False = the SSG_MFMA_SPLIT=0 descriptor); k32: ssg_conv_set_k32_mode; bnpart: statistics rows wanted; ws: expected split-K slab
# count (0 = the launch does not split; a workspace is offered exactly where the library asks for one); aff: in_act of a fused
# input transform or None; bwd: bwd_act of the backward-statistics epilogue or None; kid / fmt / body: the literals the library
# must name (fmt = ssg_conv2d_split_bn, body = ssg_conv_dma_body or None); entry: 'f32' | 'igemm'; stat: the case also runs class
# (b) and the RMS gate of class (c).
CvCase = namedtuple('CvCase', 'name op N H W C1 C2 Cout k stride cls bias res act ld1 ld2 ldo ldr c_lo ctot cred_real split k32 '
                              'bnpart ws aff bwd kid fmt body entry stat')
Geom = namedtuple('Geom', 'pad dH dW OH OW GH GW in_s out_s oy ox taps groups Cin cred_real kmode Kp R row0 transpose ld1 ld2 ldo ldr P')


def _classes(k, s, p):
    """(py, px, [(ky, kx, dy, dx)]) per output parity class of a strided input gradient (ops._conv_dgrad_impl)."""
    out = []
    for py in range(s):
        for px in range(s):
            out.append((py, px, [(ky, kx, (py + p - ky) // s, (px + p - kx) // s) for ky in range(k) for kx in range(k)
                                 if (py + p - ky) % s == 0 and (px + p - kx) % s == 0]))
    return out


def geom(c, mirrored=True, wrong_tap=False):
    """The launch geometry.  groups: [(py, px, GHq, GWq, [tap indices])] -- the accumulator sets of the launch (one, except the
    merged parity launch: four, each on its own grid ceil((OH - py) / 2) x ceil((OW - px) / 2) at output phase (py, px)).
    mirrored=False / wrong_tap: planted defects (dgrad taps as the forward's; tap 0 one column to the right)."""
    p = c.k // 2
    oh, ow = (c.H + 2 * p - c.k) // c.stride + 1, (c.W + 2 * p - c.k) // c.stride + 1
    Cin = c.C1 + c.C2
    if c.op == 'fwd':
        taps = [(ky, kx, ky - p, kx - p) for ky in range(c.k) for kx in range(c.k)]
        dH, dW, OH, OW, GH, GW, in_s, out_s, oy, ox = c.H, c.W, oh, ow, oh, ow, c.stride, 1, 0, 0
        groups = [(0, 0, GH, GW, list(range(len(taps))))]
        R, row0, tr = c.Cout, 0, 0
    else:
        dH, dW, OH, OW, in_s = oh, ow, c.H, c.W, 1
        R, row0, tr = c.ctot, c.c_lo, 1
        if c.stride == 1:
            taps = [(ky, kx, (p - ky) if mirrored else (ky - p), (p - kx) if mirrored else (kx - p)) for ky in range(c.k) for kx in range(c.k)]
            GH, GW, out_s, oy, ox = c.H, c.W, 1, 0, 0
            groups = [(0, 0, GH, GW, list(range(len(taps))))]
        elif c.cls == 'merge':
            cl = _classes(c.k, c.stride, p)
            taps, groups = [], []
            for py, px, ts in cl:
                groups.append((py, px, (c.H - py + 1) // 2, (c.W - px + 1) // 2, list(range(len(taps), len(taps) + len(ts)))))
                taps += ts
            GH, GW, out_s, oy, ox = (c.H + 1) // 2, (c.W + 1) // 2, 2, 0, 0
        else:
            py, px = c.cls
            taps = _classes(c.k, c.stride, p)[2 * py + px][2]
            GH, GW, out_s, oy, ox = (c.H - py + 1) // 2, (c.W - px + 1) // 2, 2, py, px
            groups = [(0, 0, GH, GW, list(range(len(taps))))]
    if wrong_tap:
        ky, kx, dy, dx = taps[0]
        taps = [(ky, kx, dy, dx + 1)] + taps[1:]
    kmode = 0 if Cin % 16 == 0 and c.C1 % 16 == 0 else 1
    Kp = len(taps) * Cin if kmode == 0 else cdiv(len(taps) * Cin, 16) * 16
    return Geom(p, dH, dW, OH, OW, GH, GW, in_s, out_s, oy, ox, taps, groups, Cin, c.cred_real or Cin, kmode, Kp, R, row0, tr,
                c.ld1 or c.C1, c.ld2 or c.C2, c.ldo or pad4(c.Cout), c.ldr or pad4(c.Cout), c.N * GH * GW)


def epilogue_roundings(c):
    """e of the hard gate: bias add, residual add, the leaky multiply, the mask multiply of bwd_x (slope 1/4 or 0: exact, counted anyway)."""
    return int(c.bias) + int(c.res) + int(c.act == ACT_LRELU) + int(c.bwd is not None)


# ============================================================================ 2. the weight packs, restated (include/ssunet_hip.h)
def pack_f32(w_oihw, transpose, taps, kmode, cred_pad, Kp, sigma=None):
    """ssg_pack_weights_f32 / _scaled_f32: [R][Kp] fp32, R = I (transpose) or O; reduced channel c of tap t (kernel position
    (ky[t], kx[t])) at k = (c / 16) ntaps 16 + t 16 + c % 16 (kmode 0) or t Cred_pad + c (kmode 1); channels >= the real count and
    k >= ntaps Cred_pad hold zeros.  sigma: every weight times fl(1 / sigma) (one fp32 reciprocal, one fp32 product)."""
    w = f32(w_oihw)
    O, I = w.shape[:2]
    R, cred = (I, O) if transpose else (O, I)
    nt = len(taps)
    out = np.zeros((R, Kp), dtype=F32)
    cc = np.arange(cred)
    for t, (ky, kx, _, _) in enumerate(taps):
        m = w[:, :, ky, kx]                                     # [O, I]
        m = m.T if transpose else m                              # [R, cred]
        if sigma is not None:
            m = m * (F32(1) / F32(sigma))
        k = (cc // 16) * nt * 16 + t * 16 + cc % 16 if kmode == 0 else t * cred_pad + cc
        out[:, k] = m
    return out


def _bf16_bits(a):
    """The 16 bits of an fp32 array of bf16-representable values."""
    u = f32(a).view(np.uint32)
    assert not (u & np.uint32(0xFFFF)).any()
    return (u >> np.uint32(16)).astype(np.uint16)


def pack_split(wp, BN):
    """ssg_pack_weights_split_bf16x3 of the kmode-0 rows wp [R][Kp] for column tile BN = 64 / 128: uint16 [ceil(R / BN)][Kp / 16]
    [BN][48] -- per row and 16-channel K-step 96 bytes = six 16-byte slots; slot (2 p + h) ^ ((row >> 3) & 1) holds bf16 term p
    (0..2) of channels 8 h .. 8 h + 7 of the step (mfma_split.h: the halves of a plane swap in every other group of 8 rows); rows
    beyond R are zeros."""
    R, Kp = wp.shape
    nt, ns = cdiv(R, BN), Kp // 16
    planes = [_bf16_bits(p) for p in split3(wp)]
    out = np.zeros((nt * BN, ns, 6, 8), dtype=np.uint16)
    f = (np.arange(R) >> 3) & 1
    for p in range(3):
        pl = planes[p].reshape(R, ns, 2, 8)
        for h in range(2):
            slot = (2 * p + h) ^ f                               # [R]
            out[np.arange(R)[:, None], np.arange(ns)[None, :], slot[:, None]] = pl[:, :, h]
    return out.reshape(nt, BN, ns, 48).transpose(0, 2, 1, 3).copy()


def pack_split_k32(wp, code):
    """... for the k32 formats 1016 / 1032 / 1064 / 1128 (bn = code - 1000; 9 taps): uint16 [ceil(R / bn)][Kp / 32 steps = chunk32 9
    + tap][bn / 16 fragments][3 planes][64 lanes][8] -- lane l of fragment j holds row j 16 + (l & 15), channels chunk32 32 +
    (l >> 4) 8 .. + 7 of the step's tap; rows beyond R (the narrow tiles) are zeros."""
    bn = code - 1000
    R, Kp = wp.shape
    nt, ns = cdiv(R, bn), Kp // 32
    assert Kp % 288 == 0
    w4 = f32(wp).reshape(R, Kp // 144, 9, 16)                   # [row][chunk16][tap][c]
    w5 = w4.reshape(R, ns // 9, 2, 9, 2, 8).transpose(0, 1, 3, 2, 4, 5).reshape(R, ns, 4, 8)      # [row][chunk32 9 + tap][g = (l >> 4)][8]
    planes = [_bf16_bits(p) for p in split3(w5)]
    out = np.zeros((nt * bn, ns, 3, 4, 8), dtype=np.uint16)
    for p in range(3):
        out[:R, :, p] = planes[p]
    # [tile][rl = j 16 + l15][s][p][g][8] -> [tile][s][j][p][g][l15][8]
    out = out.reshape(nt, bn // 16, 16, ns, 3, 4, 8).transpose(0, 3, 1, 4, 5, 2, 6)
    return np.ascontiguousarray(out).reshape(nt, ns, bn // 16, 3, 64, 8)


def split_pack_bytes(R, Kp, fmt):
    bn = fmt - 1000 if fmt >= 1000 else fmt
    return cdiv(R, bn) * (Kp // 16) * bn * 96


# ============================================================================ 3. the fp64 reference
Data = namedtuple('Data', 'x1 x2 w bias res scale shift bx bscale bshift bmean')
Ref = namedtuple('Ref', 'out pre acc mag magt written mask colsum')


def x_operand(c, d, wrong_sign=False):
    """X [N, dH, dW, Cin] fp32: in1 (through act_in(fl32(fma(x, scale, shift))) where the case fuses the transform) | in2."""
    x1 = f32(d.x1)
    if c.aff is not None:
        with np.errstate(all='ignore'):
            x1 = act32(preact_emul(x1, d.scale, d.shift), c.aff, wrong_sign=wrong_sign)
    return x1 if d.x2 is None else np.concatenate([x1, f32(d.x2)], axis=-1)


def tap_weights(c, g, w, transposed_kykx=False):
    """Wt [ntaps][Cin][Cout] fp32: the weight the launch multiplies channel ci of tap t by for output column co (zero rows for pad channels)."""
    w = f32(w)
    Wt = np.zeros((len(g.taps), g.Cin, c.Cout), dtype=F32)
    for t, (ky, kx, _, _) in enumerate(g.taps):
        if transposed_kykx:
            ky, kx = kx, ky
        Wt[t, :g.cred_real] = w[:, :, ky, kx].T if c.op == 'fwd' else w[:, c.c_lo:c.c_lo + c.Cout, ky, kx]
    return Wt


def _padded(X, g, GH, GW, in_s, padval=None):
    N, H, W, Cin = X.shape
    HP, WP = max(H, (GH - 1) * in_s + 6) + 4, max(W, (GW - 1) * in_s + 6) + 4
    Xp = np.zeros((N, HP, WP, Cin), dtype=X.dtype)
    if padval is not None:
        Xp[:] = padval
    Xp[:, 2:2 + H, 2:2 + W] = X
    return Xp


def _tap_view(Xp, GH, GW, in_s, dy, dx):
    return Xp[:, 2 + dy:2 + dy + (GH - 1) * in_s + 1:in_s, 2 + dx:2 + dx + (GW - 1) * in_s + 1:in_s]


def _scatter(img, val, g, py, px, GHq, GWq):
    """val [N, GHq, GWq, C] to the pixels (gy out_s + oy + py, gx out_s + ox + px) of img [N, OH, OW, C]."""
    img[:, g.oy + py:g.oy + py + (GHq - 1) * g.out_s + 1:g.out_s, g.ox + px:g.ox + px + (GWq - 1) * g.out_s + 1:g.out_s] = val


def _gather(img, g, py, px, GHq, GWq):
    return img[:, g.oy + py:g.oy + py + (GHq - 1) * g.out_s + 1:g.out_s, g.ox + px:g.ox + px + (GWq - 1) * g.out_s + 1:g.out_s]


def act64(z, act, slope=LRELU_SLOPE):
    if act == ACT_RELU:
        return np.where(z < 0, 0.0, z)
    if act == ACT_LRELU:
        return np.where(z > 0, z, z * slope)
    return z


def bwd_mask(c, d):
    """act'(fl32(fma(bwd_x, scale, shift))) as the kernel takes it: 1 where z > 0, else the slope (leaky), 0 (ReLU) or 1 (none)."""
    z = preact_emul(d.bx, d.bscale, d.bshift)
    low = {ACT_NONE: 1.0, ACT_RELU: 0.0, ACT_LRELU: LRELU_SLOPE}[c.bwd]
    return np.where(z > 0, 1.0, low), z


def conv_ref(c, d, elementwise=False, grid=None):
    """The launch of case c on data d in fp64, from the contract of ssg_conv_desc: acc = sum_t sum_c in[n, gy in_sy + dy[t], gx in_sx
    + dx[t], c] w[co, k(t, c)] with zeros outside the image (of the ACTIVATED tensor where in_scale is on), pre = acc + bias + res,
    out = act(pre) -- or, with bwd_x, out = acc act'(bwd_x scale + shift) -- at pixel (gy out_sy + out_oy, gx out_sx + out_ox) of the
    OH x OW image; every other pixel is `written` False and NaN.  mag = sum |in| |w|, magt = mag + |bias| + |res|.  colsum: the fp64
    column sums (sum v, sum v^2) of v = acc + bias over the grid -- or (sum g, sum g (x - mean)) with bwd_x.  The products of fp32
    values are exact in fp64; a K-term sum errs by at most K 2^-53 mag.  elementwise: channels with a non-finite operand go without BLAS (0 * inf = NaN is
    then certainly IEEE's).  grid: (GH, GW) override of the one accumulator set (tile_spread: the grid rounded up to whole tiles)."""
    g = geom(c)
    X = x_operand(c, d).astype(F64)
    Wt = tap_weights(c, g, d.w).astype(F64)
    shape = (c.N, g.OH, g.OW, c.Cout) if grid is None else (c.N, grid[0], grid[1], c.Cout)
    acc = np.full(shape, np.nan); mag = np.full(shape, np.nan); written = np.zeros(shape, dtype=bool)
    # elementwise: the channels that hold a non-finite activation or weight are multiplied out one by one, the others (finite) by BLAS
    special = np.flatnonzero(~np.isfinite(X).all(axis=(0, 1, 2)) | ~np.isfinite(Wt).all(axis=(0, 2))) if elementwise else np.zeros(0, dtype=int)
    plain = np.setdiff1d(np.arange(g.Cin), special)
    # a channel that is zero everywhere adds exact zeros to acc and mag (its weights are finite: a non-finite one is `special`): left out,
    # which makes the one-product class cheap at the large grids
    plain = plain[(X[..., plain] != 0).any(axis=(0, 1, 2))]
    with np.errstate(all='ignore'):
        for py, px, GHq, GWq, tis in g.groups:
            if grid is not None:
                GHq, GWq = grid
            Xp = _padded(X, g, GHq, GWq, g.in_s)
            a = np.zeros((c.N, GHq, GWq, c.Cout)); m = np.zeros_like(a)
            if not len(special) and len(plain) * len(tis) <= 288:       # short reductions: the taps side by side, one product
                xs = np.concatenate([_tap_view(Xp, GHq, GWq, g.in_s, g.taps[t][2], g.taps[t][3])[..., plain] for t in tis], axis=-1)
                ws = np.concatenate([Wt[t][plain] for t in tis], axis=0)
                a = xs @ ws; m = np.abs(xs) @ np.abs(ws)
                tis = []
            for t in tis:
                xt = np.ascontiguousarray(_tap_view(Xp, GHq, GWq, g.in_s, g.taps[t][2], g.taps[t][3]))
                if len(special):
                    for ci in special:
                        pr = xt[..., ci:ci + 1] * Wt[t, ci]
                        a += pr; m += np.abs(pr)
                if len(plain) < g.Cin:
                    xt = np.ascontiguousarray(xt[..., plain])
                a += xt @ Wt[t][plain]; m += np.abs(xt) @ np.abs(Wt[t][plain])
            if grid is not None:
                acc, mag = a, m
            else:
                _scatter(acc, a, g, py, px, GHq, GWq); _scatter(mag, m, g, py, px, GHq, GWq); _scatter(written, True, g, py, px, GHq, GWq)
        v = acc + (f32(d.bias).astype(F64) if c.bias else 0.0)
        if grid is not None:
            return Ref(None, None, v, mag, None, None, None, None)
        pre = v + (f32(d.res).astype(F64) if c.res else 0.0)
        magt = mag + (np.abs(f32(d.bias).astype(F64)) if c.bias else 0.0) + (np.abs(f32(d.res).astype(F64)) if c.res else 0.0)
        mask = None
        if c.bwd is not None:
            mask, _ = bwd_mask(c, d)
            out = pre * mask
            gg = np.where(written, out, 0.0)
            colsum = (gg.sum(axis=(0, 1, 2)), (gg * (f32(d.bx).astype(F64) - f32(d.bmean).astype(F64))).sum(axis=(0, 1, 2)))
        else:
            out = act64(pre, c.act)
            vv = np.where(written, v, 0.0)
            colsum = (vv.sum(axis=(0, 1, 2)), (vv * vv).sum(axis=(0, 1, 2)))
    return Ref(out, pre, acc, mag, magt, written, mask, colsum)


# ============================================================================ 4. gates
# The six-product split of mfma_split.h is the one analysed beside wgrad_ref.product_gate: x = x1 + x2 + x3, w = w1 + w2 + w3 in bf16
# terms, products w3 x1, w2 x2, w1 x3, w2 x1, w1 x2, w1 x1 -- the analysis is symmetric in the two operands, so C_SPLIT = 8 carries
# over with w in place of d; with one operand a power of two the sum is exact.  product_gate is wgrad_ref's.
#
# (c) hard gate.  K = ntaps Cin products are summed in an order fixed by the route (K-steps, the matrix unit's own order, the slabs
# of split-K, which partition the same K additions and add no term): each addition rounds a partial sum bounded by mag -- K u32 mag
# for any order; one more u32 mag covers the second order and the reference's own K 2^-53 mag; every product carries c u32 |x w|
# with c = C_SPLIT on split routes and 1 otherwise (an fp32 fma rounds once; exact inside the fp32 matrix unit); a fused input
# transform rounds x once more: xf u32 mag.  The epilogue then rounds e times (bias, residual, leaky or mask multiply), each a
# value bounded by magt = mag + |bias| + |res|; u32 |ref| is the final store.
def hard_gate(c, g, ref):
    K = len(g.taps) * g.Cin
    cs = C_SPLIT if c.kid in SPLIT_IDS else 1.0
    xf = 1.0 if c.aff is not None else 0.0
    with np.errstate(invalid='ignore'):
        return (K + 1 + cs + xf) * U32 * ref.mag + epilogue_roundings(c) * U32 * ref.magt + U32 * np.abs(ref.out)


def judge(c, g, ref, got, gate):
    """(worst |got - ref| / gate over the written pixels, share of elements that used the activation tie).  An element whose fp64
    pre-activation lies within the gate of 0 may take either branch of the epilogue activation.  The mask of bwd_x gets no such
    allowance: z = fl(fma(x, scale, shift)) is restated exactly (bwd_mask), so its sign is the kernel's; bwd_ties only counts the
    elements decided within rounding of z = 0, for the 1 % cap."""
    w = ref.written
    err = np.abs(got.astype(F64) - ref.out)
    tie = np.zeros(w.shape, dtype=bool)
    if c.act != ACT_NONE:
        tie = w & (np.abs(ref.pre) <= gate)
        low = LRELU_SLOPE if c.act == ACT_LRELU else 0.0
        other = np.where(ref.pre > 0, ref.pre * low, ref.pre)      # the branch act64 did not take
        err = np.where(tie, np.minimum(err, np.abs(got.astype(F64) - other)), err)
    return worst_ratio(err[w], gate[w]), float(tie[w].mean()) if w.any() else 0.0


def bwd_ties(c, d, ref):
    """Share of the written elements whose mask is decided within rounding of z = 0."""
    _, z = bwd_mask(c, d)
    zz = np.abs(f32(d.bx).astype(F64) * f32(d.bscale).astype(F64)) + np.abs(f32(d.bshift).astype(F64))
    return float((np.abs(z.astype(F64)) <= 2 * U32 * zz)[ref.written].mean())


# Statistics rows.  conv_halo_epilogue.h (and the k32 epilogue) sum, per lane or 16-lane group, fp32 DEVIATIONS dv = fl(v - pivot)
# from a pivot that is one of, or a mean of, the tile's own values of the column (pixels of the tile beyond the grid included: their
# accumulators exist), and recombine in fp64: S1 = s1 + n c, S2 = s2 + 2 c s1 + n c^2.  Every fp32 chain has at most L = th tw terms:
#   s1: each dv errs by u32 |dv|, each of < L additions by u32 sum |dv|:   |err S1| <= (L + 1) u32 sum |dv|
#   s2: dv^2 errs by 3 u32 dv^2 (dv twice, the square once), the additions by L u32 sum dv^2; 2 c s1 carries s1's error:
#       |err S2| <= (L + 3) u32 sum dv^2 + 2 |c| (L + 1) u32 sum |dv|
# with |dv| <= spread_t (max - min of the column over the whole tile) and |c| <= amax_t (max |v| over the whole tile): relative to
# sum |v - pivot| and sum (v - pivot)^2, not to sum |v|.  The fp64 recombination and the fp64 sum over tiles add 2^-50 of the sums of
# magnitudes.  The totals are judged against the fp64 column sums OF THE FP32 OUTPUT THE KERNEL WROTE (no res, no act: out = v).
def tile_spread(c, d):
    """(cnt, spread, amax) [tiles, Cout] bounding the kernel's v = acc + bias over the launch grid rounded up to whole statistics tiles."""
    g = geom(c)
    th, tw = STAT_TILE[c.kid]
    ty, tx = cdiv(g.GH, th), cdiv(g.GW, tw)
    r = conv_ref(c, d, grid=(ty * th, tx * tw))
    v = r.acc.reshape(c.N, ty, th, tx, tw, c.Cout).transpose(0, 1, 3, 2, 4, 5).reshape(c.N * ty * tx, th * tw, c.Cout)
    yy = (np.arange(ty)[:, None] * th + np.arange(th)[None, :]) < g.GH
    xx = (np.arange(tx)[:, None] * tw + np.arange(tw)[None, :]) < g.GW
    cnt = (yy.sum(axis=1)[:, None] * xx.sum(axis=1)[None, :]).reshape(-1)
    cnt = np.tile(cnt, c.N)[:, None] + np.zeros((1, c.Cout))
    # the kernel's fp32 v differs from this fp64 v by at most the hard gate of the element (hard_gate with e = the bias add): the spread of
    # the kernel's values exceeds the reference's by at most twice the tile's largest gate, its largest magnitude by once that
    K = len(g.taps) * g.Cin
    cs = C_SPLIT if c.kid in SPLIT_IDS else 1.0
    hg = (K + 1 + cs + (1.0 if c.aff is not None else 0.0) + int(c.bias)) * U32 * (r.mag + (np.abs(f32(d.bias).astype(F64)) if c.bias else 0.0)) + U32 * np.abs(r.acc)
    hg = hg.reshape(c.N, ty, th, tx, tw, c.Cout).transpose(0, 1, 3, 2, 4, 5).reshape(c.N * ty * tx, th * tw, c.Cout).max(axis=1)
    return cnt, v.max(axis=1) - v.min(axis=1) + 2 * hg, np.abs(v).max(axis=1) + hg


def stats_gates(c, d, out32):
    """(gate S1, gate S2) [Cout] for the totals of the bnpart rows of a forward-statistics case; out32 = the fp32 output judged against."""
    th, tw = STAT_TILE[c.kid]
    L = th * tw
    cnt, spread, amax = tile_spread(c, d)
    v = np.asarray(out32, dtype=F64).reshape(-1, c.Cout)
    g1 = (L + 1) * U32 * (cnt * spread).sum(axis=0) + 2.0 ** -50 * np.abs(v).sum(axis=0)
    g2 = ((L + 3) * U32 * (cnt * spread * spread).sum(axis=0) + 2 * (L + 1) * U32 * (cnt * amax * spread).sum(axis=0)
          + 2.0 ** -50 * (v * v).sum(axis=0))
    return g1, g2


# Backward statistics (conv_igemm_halo_k32.hip, BWD): plain fp32 sums of g and of fl(g fl(x - mean)) inside a wave's rows (chains of
# at most L = th tw terms), fp64 beyond:  |err S1| <= L u32 sum |g|,  |err S2| <= (L + 2) u32 sum |g (x - mean)|.
def bwd_stats_gates(c, d, out32, written):
    th, tw = STAT_TILE[c.kid]
    L = th * tw
    gg = np.where(written, np.asarray(out32, dtype=F64), 0.0)
    xm = f32(d.bx).astype(F64) - f32(d.bmean).astype(F64)
    return (L * U32 * np.abs(gg).sum(axis=(0, 1, 2)) + 1e-300, (L + 2) * U32 * np.abs(gg * xm).sum(axis=(0, 1, 2)) + 1e-300)


def stats_of_output(c, d, out32, written):
    """The fp64 column sums the rows must total: (sum v, sum v^2), or (sum g, sum g (x - mean)) with bwd_x, of the fp32 output."""
    gg = np.where(written, np.asarray(out32, dtype=F64), 0.0)
    if c.bwd is not None:
        return gg.sum(axis=(0, 1, 2)), (gg * (f32(d.bx).astype(F64) - f32(d.bmean).astype(F64))).sum(axis=(0, 1, 2))
    return gg.sum(axis=(0, 1, 2)), (gg * gg).sum(axis=(0, 1, 2))


def equal_values(got, ref, where):
    got = np.asarray(got).astype(F64)
    return bool(np.all(got[where] == ref[where]))


def first_mismatch(got, ref, where):
    got = np.asarray(got).astype(F64)
    bad = np.argwhere(where & ~(got == ref))
    if not len(bad):
        return None
    i = tuple(int(v) for v in bad[0])
    return '%d of %d elements differ, first at (n, y, x, co) = %s: got %r, reference %r' % (len(bad), int(where.sum()), i, got[i], ref[i])


def one_product_gate(c, g, ref):
    """(b) `full`: every element is one product p (= ref.acc) and the epilogue: c u32 |p| (wgrad_ref.product_gate: c = 8 on split routes,
    one rounding otherwise), one more u32 |p| for the rounding of a fused input transform, and the epilogue's e roundings as in hard_gate."""
    e = epilogue_roundings(c)
    with np.errstate(invalid='ignore'):
        return (product_gate(ref.acc, c.kid in SPLIT_IDS) + (U32 * np.abs(ref.acc) if c.aff is not None else 0.0)
                + e * U32 * ref.magt + (U32 * np.abs(ref.out) if e else 0.0))


# ============================================================================ 5. data
def _seed(c, cls):
    return (sum(ord(ch) * (i + 1) for i, ch in enumerate(c.name)) * 7 + cls * 1009) % (2 ** 31)


def _shapes(c, g):
    """(x1, x2, w, img) shapes: img = [N, OH, OW, Cout] of out / res / bwd_x."""
    w = (c.Cout, g.cred_real, c.k, c.k) if c.op == 'fwd' else (g.cred_real, c.ctot, c.k, c.k)
    return (c.N, g.dH, g.dW, c.C1), (c.N, g.dH, g.dW, c.C2), w, (c.N, g.OH, g.OW, c.Cout)


def irange(c, g):
    """Class (a): |x| <= irange, |w| <= 2 (one bf16 term, so that the three products the split leaves out vanish), |bias|, |res| <=
    1000.  Split routes take x up to 2^17 (three bf16 terms) where K allows: K r 2 <= 2^21, a quarter of that under a fused input
    transform (|X| <= 2 r + 3, in units of 1/4 with the leaky slope).  int_class_is_exact asserts the bound from mag."""
    K = len(g.taps) * g.Cin
    if c.kid not in SPLIT_IDS:
        return 8
    r = min(1 << 17, (1 << 20) // K)
    return max(r // 4, 2) if c.aff is not None else r


def _zero_pad_channels(x1, x2, c, g):
    """Pad channels (>= cred_real, always at the end of the one input of such a case) hold zeros, as the NHWC contract says."""
    if g.cred_real < g.Cin:
        assert c.C2 == 0
        x1[..., g.cred_real:] = 0
    return x1, x2


def int_data(c):
    g = geom(c)
    rng = np.random.RandomState(_seed(c, 1))
    s1, s2, sw, si = _shapes(c, g)
    r = irange(c, g)
    x1 = f32(rng.randint(-r, r + 1, s1)); x2 = f32(rng.randint(-r, r + 1, s2)) if c.C2 else None
    x1, x2 = _zero_pad_channels(x1, x2, c, g)
    w = f32(rng.randint(-2, 3, sw))
    bias = f32(rng.randint(-1000, 1001, c.Cout)) if c.bias else None
    res = f32(rng.randint(-1000, 1001, si)) if c.res else None
    sc = sh = bx = bsc = bsh = bmu = None
    if c.aff is not None:      # scale in {1, 2, -1}, integer shift > 0: a transformed padding pixel would be act(shift) != 0
        sc, sh = f32(rng.choice([1.0, 2.0, -1.0], c.C1)), f32(rng.randint(1, 4, c.C1))
    if c.bwd is not None:      # z = x scale + shift is an odd multiple of 1/2: never 0
        bx = f32(rng.randint(-8, 9, si)); bsc = f32(rng.choice([1.0, 2.0, -1.0], c.Cout)); bsh = f32(rng.randint(-3, 4, c.Cout) + 0.5)
        bmu = f32(rng.randint(-2, 3, c.Cout))
    return Data(x1, x2, w, bias, res, sc, sh, bx, bsc, bsh, bmu)


def int_class_is_exact(c, ref):
    """Class (a): sum |terms| < 2^24 in units of the smallest term (1, or 1/4 where a leaky slope is involved)."""
    unit = 0.25 if ACT_LRELU in (c.act, c.aff, c.bwd) else 1.0
    return float(np.nanmax(ref.magt)) / unit < 2 ** 24


def rand_data(c):
    """Class (c): full-mantissa operands with non-zero means; weights scaled by K^-1/2 so that the outputs are O(1)."""
    g = geom(c)
    rng = np.random.RandomState(_seed(c, 3))
    s1, s2, sw, si = _shapes(c, g)
    K = len(g.taps) * g.Cin
    x1 = _full(rng, s1, 0.3); x2 = _full(rng, s2, -0.2) if c.C2 else None
    x1, x2 = _zero_pad_channels(x1, x2, c, g)
    w = _fullw(rng, sw, K)
    bias = _full(rng, (c.Cout,), 0.2) if c.bias else None
    res = _full(rng, si, -0.1) if c.res else None
    sc = sh = bx = bsc = bsh = bmu = None
    if c.aff is not None:
        sc = f32(rng.uniform(0.5, 1.5, c.C1) * rng.choice([1.0, -1.0], c.C1)); sh = f32(rng.uniform(0.1, 0.6, c.C1))
    if c.bwd is not None:
        bx = _full(rng, si, 0.4); bsc = f32(rng.uniform(0.5, 1.5, c.Cout) * rng.choice([1.0, -1.0], c.Cout))
        bsh = f32(rng.uniform(-0.5, 0.5, c.Cout)); bmu = f32(rng.uniform(0.2, 0.6, c.Cout))
    return Data(x1, x2, w, bias, res, sc, sh, bx, bsc, bsh, bmu)


def _fullw(rng, shape, K):
    a = f32((0.1 + rng.standard_normal(shape)) / np.sqrt(K))
    return (a.view(np.uint32) | np.uint32(1)).view(np.float32)


def onehot_site(c):
    """(n, y, x, ci) of the one non-zero input element: the last image, a middle row, the last column but one, and a channel of in2
    where there is one (else the last real channel)."""
    g = geom(c)
    ci = c.C1 + c.C2 // 2 if c.C2 else g.cred_real - 1
    return c.N - 1, g.dH // 2, max(g.dW - 2, 0), ci


def onehot_data(c, variant):
    """Class (b): the input is non-zero at one pixel and channel, so every output element is one product (or none) and the epilogue.
    variant 'xpow2': x a power of two -> the result is the correctly rounded w 2^k (+ bias); 'wpow2': weights powers of two;
    'full': both at full mantissa.  Bias, activation and bwd_x stay on; the residual is zero (a second rounding behind the bias would
    make `exact` ambiguous).  A fused input transform stays on with shift 0, so that the zero pixels stay zero: its scale is a signed
    power of two, or at `full` a full-mantissa value (X = fl(x scale): the one rounding the gate allows for)."""
    g = geom(c)
    rng = np.random.RandomState(_seed(c, 2))
    s1, s2, sw, si = _shapes(c, g)
    K = len(g.taps) * g.Cin
    n, y, x, ci = onehot_site(c)
    x1 = np.zeros(s1, dtype=F32); x2 = np.zeros(s2, dtype=F32) if c.C2 else None
    val = _pow2(rng, (1,))[0] if variant == 'xpow2' else _full(rng, (1,), 0.3)[0]
    w = _pow2(rng, sw) if variant == 'wpow2' else _fullw(rng, sw, K)
    sc = sh = bx = bsc = bsh = bmu = None
    if c.aff is not None:
        sc = _full(rng, (c.C1,), 0.7) if variant == 'full' else _pow2(rng, (c.C1,))
        sh = np.zeros(c.C1, dtype=F32)
        val = F32(abs(val) * np.sign(sc[ci]))                  # x scale > 0: a ReLU transform keeps the one product
    if ci >= c.C1:
        x2[n, y, x, ci - c.C1] = val
    else:
        x1[n, y, x, ci] = val
    res = np.zeros(si, dtype=F32) if c.res else None
    bias = _full(rng, (c.Cout,), 0.2) if c.bias else None
    if c.bwd is not None:
        bx = _full(rng, si, 0.4); bsc = f32(rng.uniform(0.5, 1.5, c.Cout) * rng.choice([1.0, -1.0], c.Cout))
        bsh = f32(rng.uniform(-0.5, 0.5, c.Cout)); bmu = f32(rng.uniform(0.2, 0.6, c.Cout))
    return Data(x1, x2, w, bias, res, sc, sh, bx, bsc, bsh, bmu)


def nonfinite_data(c, where):
    """rand_data with one +inf, one NaN and one 3.4e38 planted in x (in1) or in w."""
    g = geom(c)
    d = rand_data(c)
    x1 = d.x1.copy(); w = d.w.copy()
    for i, v in enumerate((np.inf, np.nan, 3.4e38)):
        if where == 'x':
            x1[c.N - 1, (g.dH // 2 + i) % g.dH, (g.dW - 2 + i) % g.dW, (5 + 17 * i) % min(c.C1, g.cred_real)] = v
        else:
            w[(3 + 13 * i) % w.shape[0], (5 + 17 * i) % w.shape[1], i % c.k, (i + 1) % c.k] = v
    return d._replace(x1=x1, w=w)


# ============================================================================ 6. the descriptor of a case
def fill_desc(D, c, a, ky_kx=False):
    """Fill the ssg_conv_desc D (a fresh _lib.ConvDesc) for case c from the address dict a (in1 in2 w bias res out scale shift bx
    bscale bshift bmean: the ones the case uses; w = the address of row 0 of the pack: the slice offset is added here).  bnpart, ws and
    w_split are the caller's, in the order ops._conv_launch sets them."""
    g = geom(c)
    D.in1 = a['in1']; D.C1 = c.C1; D.ld1 = g.ld1
    if c.C2:
        D.in2 = a['in2']; D.C2 = c.C2; D.ld2 = g.ld2
    D.N, D.H, D.W = c.N, g.dH, g.dW
    D.w = a['w'] + g.row0 * g.Kp * 4; D.Kp = g.Kp; D.kmode = g.kmode
    D.bias = a['bias'] if c.bias else None
    if c.res:
        D.res = a['res']; D.ldr = g.ldr
    D.out = a['out']; D.Cout = c.Cout; D.ldo = g.ldo
    D.GH, D.GW, D.OH, D.OW = g.GH, g.GW, g.OH, g.OW
    D.in_sy = D.in_sx = g.in_s; D.out_sy = D.out_sx = g.out_s; D.out_oy, D.out_ox = g.oy, g.ox
    D.ntaps = len(g.taps)
    for t, (_, _, dy, dx) in enumerate(g.taps):
        D.dy[t] = dy; D.dx[t] = dx
    D.act = c.act; D.slope = LRELU_SLOPE if c.act == ACT_LRELU else 0.0
    D.parity_merge = 1 if c.cls == 'merge' else 0
    if c.aff is not None:
        D.in_scale = a['scale']; D.in_shift = a['shift']; D.in_act = c.aff; D.in_slope = LRELU_SLOPE if c.aff == ACT_LRELU else 0.0
    if c.bwd is not None:
        D.bwd_x = a['bx']; D.bwd_ldx = g.ldr; D.bwd_scale = a['bscale']; D.bwd_shift = a['bshift']; D.bwd_mean = a['bmean']
        D.bwd_act = c.bwd; D.bwd_slope = LRELU_SLOPE if c.bwd == ACT_LRELU else 0.0
    return D


def workspace_bytes(c):
    g = geom(c)
    return c.ws * g.P * pad4(c.Cout) * 4


def bnpart_rows(c):
    g = geom(c)
    if c.kid not in STAT_TILE or c.ws:
        return 0
    th, tw = STAT_TILE[c.kid]
    return c.N * cdiv(g.GH, th) * cdiv(g.GW, tw)


# ============================================================================ 7. the float32 emulation
def k_steps(c, g, tis):
    """The K-steps [(tap, c0, c1)] of one accumulator set in the route's order: kmode 0 walks the channel chunks (32 channels on the
    k32 kernels and in the split-once LDS-DMA body, else 16) and the taps inside a chunk; kmode 1 walks the taps."""
    if g.kmode == 1:
        return [(t, 0, g.Cin) for t in tis]
    ch = 32 if (c.kid in K32_IDS or c.body == 2) else 16
    return [(t, c0, min(c0 + ch, g.Cin)) for c0 in range(0, g.Cin, ch) for t in tis]


_TERMS = ((2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0))      # (w term, x term): w3 x1, w2 x2, w1 x3, w2 x1, w1 x2, w1 x1


def _accumulate(acc, xt, wt, split, drop_x3, drop_x2w2):
    """acc [P..., Cout] += xt [P..., n] . wt [n, Cout], one channel at a time in fp32."""
    for i in range(xt.shape[-1]):
        wv = wt[i]
        if not wv.any():
            continue
        xv = xt[..., i]
        if split:
            xs = list(split3(xv)); ws = split3(wv)
            if drop_x3:
                xs[2] = np.zeros_like(xs[2])
            for qw, qx in _TERMS:
                if drop_x2w2 and (qw, qx) == (1, 1):
                    continue
                acc += xs[qx][..., None] * ws[qw]
        else:
            acc[...] = (acc.astype(F64) + xv.astype(F64)[..., None] * wv.astype(F64)).astype(F32)


def _seq_sum(a):
    """fp32 sum of a [T, L, C] along L, one term at a time."""
    s = np.zeros((a.shape[0], a.shape[2]), dtype=F32)
    for l in range(a.shape[1]):
        s = s + a[:, l]
    return s


def _tiles(img, th, tw, fill):
    """img [N, GH, GW, C] -> [N ty tx, th tw, C], padded with `fill`, and the matching validity [N ty tx, th tw]."""
    N, GH, GW, C = img.shape
    ty, tx = cdiv(GH, th), cdiv(GW, tw)
    p = np.full((N, ty * th, tx * tw, C), fill, dtype=img.dtype); p[:, :GH, :GW] = img
    ok = np.zeros((N, ty * th, tx * tw), dtype=bool); ok[:, :GH, :GW] = True
    t = lambda a, c: a.reshape(N, ty, th, tx, tw, c).transpose(0, 1, 3, 2, 4, 5).reshape(N * ty * tx, th * tw, c)
    return t(p, C), t(ok[..., None], 1)[..., 0]


def emul(c, d, wrong_tap=False, kykx_transposed=False, not_mirrored=False, in2_chunk_off=False, drop_last_step=False,
         drop_last_slab=False, drop_last_col_tile=False, drop_last_row_tile=False, pad_written=False, xform_padding=False,
         lrelu_wrong_sign=False, bwd_mask_from_grad=False, parity_wrong_phase=False, drop_x3=False, drop_x2w2=False,
         unit_stride_taps=False, res_before_stats=False):
    """The launch in float32: every accumulator adds its K-steps in the order of k_steps, one channel at a time (fp32 routes: one
    fused multiply-add per channel; split routes: the six bf16-term products of mfma_split.h, small ones first, each added in fp32);
    split-K (c.ws slabs over the 16-channel chunks, ceil(chunks / slabs) each) adds the slabs in order; then bias, residual and
    activation (or the mask of bwd_x) in fp32.  Returns (out [N, OH, OW, pad4(Cout)] fp32, NaN where nothing is written and 0 in the
    pad lanes; rows [tiles, 2, Cout] fp64 of the statistics epilogue or None; v32 [N, OH, OW, Cout]: acc + bias, what the forward
    rows are statistics of).
    Defects (all off): tap 0 one column off; ky / kx transposed; dgrad taps not mirrored; in2's channels read one chunk further; the
    last K-step dropped; the last slab dropped; the last column / row of tiles not written; a pad lane written; the input transform
    applied to padding pixels; the leaky slope on the wrong sign; the mask of bwd_x taken from the gradient; parity classes (0, 1)
    and (1, 0) written at each other's phase; the third bf16 term of x dropped; the x2 w2 product dropped; stride-2 taps read at
    unit stride; the residual added before the statistics."""
    g = geom(c, mirrored=not not_mirrored, wrong_tap=wrong_tap)
    split = c.kid in SPLIT_IDS
    chunk = 32 if (c.kid in K32_IDS or c.body == 2) else 16
    if in2_chunk_off and d.x2 is not None:
        x2 = np.zeros_like(f32(d.x2)); x2[..., :c.C2 - chunk] = f32(d.x2)[..., chunk:]
        d = d._replace(x2=x2)
    X = x_operand(c, d)
    Wt = tap_weights(c, g, d.w, kykx_transposed)
    padval = None
    if xform_padding and c.aff is not None:
        padval = np.zeros(g.Cin, dtype=F32); padval[:c.C1] = act32(f32(d.shift), c.aff)
    in_s = 1 if unit_stride_taps else g.in_s
    out = np.full((c.N, g.OH, g.OW, pad4(c.Cout)), np.nan, dtype=F32)
    v32 = np.full((c.N, g.OH, g.OW, c.Cout), np.nan, dtype=F32)
    sv32 = v32.copy()                                                        # what the rows are taken from (v32 unless a defect says otherwise)
    with np.errstate(all='ignore'):
        for gi, (py, px, GHq, GWq, tis) in enumerate(g.groups):
            Xp = _padded(X, g, GHq, GWq, in_s, padval)
            steps = k_steps(c, g, tis)
            if drop_last_step:
                steps = steps[:-1]
            nsl = max(c.ws, 1)
            cps = cdiv(g.Cin // 16, nsl) if c.ws else 0
            slabs = [[s for s in steps if s[1] // 16 // cps == z] for z in range(nsl)] if c.ws else [steps]
            if drop_last_slab and c.ws:
                slabs = slabs[:-1]
            total = None
            for sl in slabs:
                acc = np.zeros((c.N, GHq, GWq, c.Cout), dtype=F32)
                for t, c0, c1 in sl:
                    xt = _tap_view(Xp, GHq, GWq, in_s, g.taps[t][2], g.taps[t][3])[..., c0:c1]
                    _accumulate(acc, xt, Wt[t, c0:c1], split, drop_x3, drop_x2w2)
                total = acc if total is None else total + acc
            v = total + f32(d.bias) if c.bias else total
            if parity_wrong_phase and len(g.groups) == 4 and gi in (1, 2):
                py, px = px, py
                GHq2, GWq2 = (g.OH - py + 1) // 2, (g.OW - px + 1) // 2
                v = v[:, :min(GHq, GHq2), :min(GWq, GWq2)]; GHq, GWq = v.shape[1], v.shape[2]
            elif parity_wrong_phase and len(g.groups) == 1 and g.out_s == 2:
                g = g._replace(oy=g.ox, ox=g.oy)
                GHq2, GWq2 = (g.OH - g.oy + 1) // 2, (g.OW - g.ox + 1) // 2
                v = v[:, :min(GHq, GHq2), :min(GWq, GWq2)]; GHq, GWq = v.shape[1], v.shape[2]
            o = v + f32(_gather(f32(d.res), g, py, px, GHq, GWq)) if c.res else v
            if c.bwd is not None:
                z = _gather(preact_emul(d.bx, d.bscale, d.bshift), g, py, px, GHq, GWq)
                low = F32({ACT_NONE: 1.0, ACT_RELU: 0.0, ACT_LRELU: LRELU_SLOPE}[c.bwd])
                o = np.where((o > 0) if bwd_mask_from_grad else (z > 0), o, o * low)
            else:
                o = act32(o, c.act, wrong_sign=lrelu_wrong_sign)
            keep = np.ones((GHq, GWq), dtype=bool)
            if (drop_last_col_tile or drop_last_row_tile) and c.kid in OUT_TILE:
                th, tw = OUT_TILE[c.kid]
                if drop_last_col_tile:
                    keep[:, (cdiv(GWq, tw) - 1) * tw:] = False
                if drop_last_row_tile:
                    keep[(cdiv(GHq, th) - 1) * th:, :] = False
            full = np.zeros((c.N, GHq, GWq, pad4(c.Cout)), dtype=F32)
            full[..., :c.Cout] = o
            if pad_written:
                full[..., c.Cout:] = F32(1)
            full = np.where(keep[None, :, :, None], full, _gather(out, g, py, px, GHq, GWq))
            _scatter(out, full, g, py, px, GHq, GWq)
            _scatter(v32, v, g, py, px, GHq, GWq)
            _scatter(sv32, (o if res_before_stats else v), g, py, px, GHq, GWq)
    rows = None
    if (c.bnpart or c.bwd is not None) and c.kid in STAT_TILE and len(g.groups) == 1:
        th, tw = STAT_TILE[c.kid]
        py, px, GHq, GWq, _ = g.groups[0]
        if c.bwd is not None:
            gt, ok = _tiles(_gather(out[..., :c.Cout], g, py, px, GHq, GWq), th, tw, F32(0))
            xm, _ = _tiles(f32(_gather(f32(d.bx), g, py, px, GHq, GWq) - f32(d.bmean)), th, tw, F32(0))
            gt = np.where(ok[..., None], gt, F32(0))
            rows = np.stack([_seq_sum(gt).astype(F64), _seq_sum(f32(gt * xm)).astype(F64)], axis=1)
        else:
            vt, ok = _tiles(_gather(sv32, g, py, px, GHq, GWq), th, tw, F32(0))
            piv = vt[:, 0]                                                  # the tile's first value of the column
            dv = np.where(ok[..., None], f32(vt - piv[:, None]), F32(0))
            s1 = _seq_sum(dv).astype(F64); s2 = _seq_sum(f32(dv * dv)).astype(F64)
            n = ok.sum(axis=1).astype(F64)[:, None]; cc = piv.astype(F64)
            rows = np.stack([s1 + n * cc, s2 + 2.0 * cc * s1 + n * cc * cc], axis=1)
    return out, rows, v32


# ============================================================================ 8. the host queries of a case, in the order ops._conv_launch asks them
Plan = namedtuple('Plan', 'kid fmt rows ws_bytes aff_ok bwd_ok body')


def plan_queries(lib, c, D, split_addr, bnpart_addr, ws_addr):
    """Complete the descriptor D (fill_desc) the way ops._conv_launch does and return what the library says about it: the split pack
    first (only where the case offers split weights), then the statistics rows, then the split-K workspace (only without bnpart and
    w_split), then the kernel id OF THE DESCRIPTOR AS LAUNCHED.  split_addr(fmt), bnpart_addr(rows), ws_addr(nbytes) supply the
    addresses (device buffers in the GPU test, dummies in the rehearsal).  Host calls only: nothing is launched or dereferenced."""
    import ctypes
    q = lambda name: lib.call(name, ctypes.byref(D))
    lib.call('ssg_conv_set_k32_mode', c.k32)
    fmt = q('ssg_conv2d_split_bn') if c.split and D.kmode == 0 else 0
    if fmt:
        D.w_split = split_addr(fmt)
    aff_ok, bwd_ok = q('ssg_conv2d_in_affine_ok'), q('ssg_conv2d_bwd_stats_ok')
    rows = q('ssg_conv2d_bnpart_rows')
    if (c.bnpart or c.bwd is not None) and rows:
        D.bnpart = bnpart_addr(rows)
    ws = 0
    if not D.bnpart and not fmt:
        ws = q('ssg_conv2d_workspace_bytes')
        if ws:
            D.ws = ws_addr(ws); D.ws_bytes = ws
    fn = lib.load().ssg_conv_dma_body
    fn.argtypes = [ctypes.POINTER(type(D))]; fn.restype = ctypes.c_int
    return Plan(q('ssg_conv2d_kernel_id'), fmt, rows, ws, aff_ok, bwd_ok, fn(ctypes.byref(D)))


def check_plan(c, p):
    """The library's answers are what the case table says (literals) and what the case needs."""
    assert p.kid == c.kid, '%s: the library names kernel id %d, the table expects %d' % (c.name, p.kid, c.kid)
    assert p.fmt == c.fmt, '%s: ssg_conv2d_split_bn %d, the table expects %d' % (c.name, p.fmt, c.fmt)
    assert p.ws_bytes == workspace_bytes(c), '%s: workspace %d bytes, the table expects %d slabs = %d' % (c.name, p.ws_bytes, c.ws, workspace_bytes(c))
    if c.kid not in (16, 42):               # the streaming 1x1 kernel and the merged parity launch take no bnpart: the rows reported are
                                            # those of the kernel a bnpart pointer would select (16) / of an 8 x 16 tile nothing writes (42)
        assert p.rows == bnpart_rows(c), '%s: %d bnpart rows, expected %d' % (c.name, p.rows, bnpart_rows(c))
    assert not (c.bnpart or c.bwd is not None) or p.rows > 0, c.name
    assert c.aff is None or p.aff_ok, c.name
    assert c.bwd is None or p.bwd_ok, c.name
    if c.body is not None:
        assert p.body == c.body, '%s: ssg_conv_dma_body %d, the table expects %d' % (c.name, p.body, c.body)


# ============================================================================ 9. the case table
def _c(name, op, N, H, W, C1, C2, Cout, kid, k=3, stride=1, cls=None, bias=False, res=False, act=ACT_NONE, ld1=None, ld2=None,
       ldo=None, ldr=None, c_lo=0, ctot=None, cred_real=None, split=True, k32=1, bnpart=False, ws=0, aff=None, bwd=None, fmt=0,
       body=None, entry='f32', stat=False):
    return CvCase(name, op, N, H, W, C1, C2, Cout, k, stride, cls, bias, res, act, ld1, ld2, ldo, ldr, c_lo,
                  ctot if ctot is not None else (Cout if op == 'dgrad' else None), cred_real, split, k32, bnpart, ws, aff, bwd, kid, fmt,
                  body, entry, stat)


R, L = ACT_RELU, ACT_LRELU


def _cases():
    cs = []
    # ---- register-staged, kmode 1 (Cin % 16 != 0): ids 0 (Cout > 64), 1 (33..64), 2 (<= 32); tiles of 8 / 16 / 16 rows x 16 columns
    cs += [_c('reg0_c24_134', 'fwd', 2, 9, 11, 24, 0, 134, 0, bias=True, res=True, act=R, ld1=28, ldo=140, ldr=144, stat=True),
           _c('reg0_cat_s2', 'fwd', 1, 19, 37, 8, 16, 130, 0, stride=2, ld2=20, act=L, bias=True),
           _c('reg0_1x1', 'fwd', 2, 9, 19, 20, 0, 72, 0, k=1, res=True),
           _c('reg0_dgrad_slice', 'dgrad', 1, 9, 19, 24, 0, 68, 0, c_lo=12, ctot=96, cred_real=22, ldo=72),
           _c('reg1_c24_40', 'fwd', 2, 17, 19, 24, 0, 40, 1, bias=True, act=L, ldo=44, stat=True),
           _c('reg1_cat', 'fwd', 1, 9, 11, 8, 12, 62, 1, ld1=12, ld2=16, res=True, act=R, ldr=68),
           _c('reg1_s2_cls', 'dgrad', 1, 13, 15, 24, 0, 36, 1, stride=2, cls=(1, 0), c_lo=4, ctot=44, cred_real=22),
           _c('reg0_cls00', 'dgrad', 1, 13, 15, 24, 0, 68, 0, stride=2, cls=(0, 0), ctot=68),
           _c('reg2_1x1_dgrad_slice', 'dgrad', 2, 9, 11, 20, 0, 12, 2, k=1, c_lo=8, ctot=24, res=True, ldo=16, ldr=20),
           _c('reg1_1x1', 'fwd', 1, 5, 33, 12, 0, 33, 1, k=1, bias=True),
           _c('reg2_c24_20', 'fwd', 2, 17, 19, 24, 0, 20, 2, bias=True, res=True, act=R, stat=True),
           _c('reg2_k0_c32_24', 'fwd', 1, 17, 33, 32, 0, 24, 2, act=L, ld1=36, ldo=28),
           _c('reg2_cat_s2', 'fwd', 2, 9, 11, 8, 8, 30, 2, stride=2, ld2=12),
           _c('reg2_dgrad_cls11', 'dgrad', 1, 9, 11, 20, 0, 12, 2, stride=2, cls=(1, 1), ctot=12, cred_real=18)]
    # ---- thin (10), thin4 (12 / 13), tiny (14): one input, unit stride, the whole image
    cs += [_c('thin_c24_3', 'fwd', 2, 9, 19, 24, 0, 3, 10, bias=True, act=R, ld1=28, ldo=8, stat=True),
           _c('thin_c20_5_1x1', 'fwd', 1, 7, 33, 20, 0, 5, 10, k=1, res=True, act=L, ldr=12),
           _c('thin_dgrad_c16_8', 'dgrad', 2, 9, 17, 16, 0, 8, 10, c_lo=4, ctot=12, cred_real=14),
           _c('thin4in_c20', 'fwd', 2, 9, 31, 4, 0, 20, 12, cred_real=3, bias=True, act=L, stat=True),
           _c('thin4in_c9_1x1', 'fwd', 1, 5, 33, 4, 0, 9, 12, k=1, cred_real=3, res=True, act=R, ld1=8, ldo=16, ldr=20),
           _c('thin4in_dgrad_c33', 'dgrad', 1, 7, 18, 4, 0, 33, 12, c_lo=3, ctot=36, cred_real=3),
           _c('thin4out_c64_3', 'fwd', 2, 9, 19, 64, 0, 3, 13, bias=True, act=R, stat=True),
           _c('thin4out_c192_5', 'fwd', 1, 7, 33, 192, 0, 5, 13, res=True, act=L, ld1=196, ldo=12, ldr=16),
           _c('thin4out_dgrad_c128_8', 'dgrad', 1, 9, 17, 128, 0, 8, 13, c_lo=2, ctot=10),
           _c('tiny_c3', 'fwd', 2, 9, 31, 4, 0, 3, 14, cred_real=3, bias=True, act=R, stat=True),
           _c('tiny_c8_ld', 'fwd', 1, 70, 67, 4, 0, 8, 14, cred_real=3, res=True, act=L, ld1=8, ldo=12, ldr=16),
           _c('tiny_dgrad_c4', 'dgrad', 1, 7, 18, 4, 0, 4, 14, c_lo=1, ctot=5, cred_real=3)]
    # ---- the large-grid routes: thin32 (15: 4 -> >= 32 channels, 3x3, W >= 32, >= 65536 pixels) and the streaming 1x1 (16: 64 ->
    # >= 32 channels, >= 65536 pixels, no bnpart).  260 x 253 = 65780 pixels: a ragged 32-pixel strip
    cs += [_c('thin32_c32', 'fwd', 1, 260, 253, 4, 0, 32, 15, cred_real=3, bias=True, act=R),
           _c('thin32_c40_ld', 'fwd', 1, 260, 253, 4, 0, 40, 15, cred_real=3, res=True, ld1=8, ldo=44, ldr=48),
           _c('thin32_dgrad_c36', 'dgrad', 1, 260, 253, 4, 0, 36, 15, ctot=36, cred_real=3),
           _c('k64_c32', 'fwd', 1, 260, 253, 64, 0, 32, 16, k=1, bias=True, act=L),
           _c('k64_c42_ld', 'fwd', 1, 260, 253, 64, 0, 42, 16, k=1, res=True, act=R, ld1=68, ldo=48, ldr=44, split=False)]
    # ---- LDS-DMA, fp32 (kmode 0, Cout > 32, not the 3x3 unit-stride window): 22 (Kp <= 256), 20 / 21 (Kp > 256, Cout > 64 / <= 64)
    cs += [_c('dma22_1x1_c32_40', 'fwd', 2, 9, 19, 32, 0, 40, 22, k=1, bias=True, res=True, act=R, ldr=48, stat=True),
           _c('dma22_1x1_cat_134', 'fwd', 1, 17, 19, 16, 32, 134, 22, k=1, ld1=20, ld2=36, ldo=140, act=L, bias=True),
           _c('dma22_bn', 'fwd', 2, 9, 19, 48, 0, 72, 22, k=1, bias=True, bnpart=True),
           _c('dma22_cls01', 'dgrad', 1, 17, 21, 32, 0, 48, 22, stride=2, cls=(0, 1), c_lo=16, ctot=80),
           _c('dma20_s2_c32_136', 'fwd', 2, 15, 19, 32, 0, 136, 20, stride=2, bias=True, act=R, stat=True),
           _c('dma20_s2_cat_bn', 'fwd', 1, 18, 36, 16, 16, 132, 20, stride=2, ld2=20, bias=True, bnpart=True),
           _c('dma20_cls11', 'dgrad', 1, 17, 21, 80, 0, 96, 20, stride=2, cls=(1, 1), c_lo=16, ctot=112, split=False),
           _c('dma20_1x1_c272_134', 'fwd', 1, 9, 19, 272, 0, 134, 20, k=1, res=True, act=L, ld1=276, ldo=140, ldr=144),
           _c('dma21_s2_cat', 'fwd', 1, 15, 19, 16, 32, 48, 21, stride=2, ld1=20, ld2=36, ldo=52, act=R),
           _c('dma21_cls11_slice', 'dgrad', 1, 17, 21, 80, 0, 40, 21, stride=2, cls=(1, 1), c_lo=8, ctot=56),
           _c('dma21_s2_c32_40', 'fwd', 2, 15, 19, 32, 0, 40, 21, stride=2, res=True, act=L, ldr=44, stat=True),
           _c('dma21_s2_bn', 'fwd', 1, 33, 35, 48, 0, 64, 21, stride=2, bnpart=True, split=False),
           _c('dma21_1x1_c272', 'fwd', 1, 9, 19, 272, 0, 34, 21, k=1, bias=True)]
    # ---- halo, fp32 (3x3 unit stride): halo16 (33 / 34: GW <= 16), the default narrow tile (32), the wide tile on a full chip (30:
    # N ceil(GH / 4) ceil(GW / 32) ceil(Cout / 128) >= 768), the long tile (31: Cout <= 64, Cin > 128, N ceil(GH / 8) ceil(GW / 32) >= 512)
    cs += [_c('halo33_c16_134', 'fwd', 2, 9, 16, 16, 0, 134, 33, bias=True, res=True, act=R, ldo=140, stat=True),
           _c('halo33_cat_bn', 'fwd', 1, 17, 11, 16, 32, 136, 33, ld1=20, bias=True, bnpart=True),
           _c('halo33_dgrad', 'dgrad', 2, 9, 13, 32, 0, 130, 33, c_lo=8, ctot=144, res=True, act=L, ldr=136),
           _c('halo34_c16_40', 'fwd', 2, 9, 16, 16, 0, 40, 34, bias=True, act=L, stat=True),
           _c('halo34_bn_w5', 'fwd', 3, 19, 5, 48, 0, 64, 34, bnpart=True, split=False),
           _c('halo34_cat_c38', 'fwd', 1, 9, 12, 16, 32, 38, 34, ld1=20, ld2=36, res=True, act=R, ldo=48, ldr=44),
           _c('halo34_dgrad_slice', 'dgrad', 1, 9, 9, 32, 0, 40, 34, c_lo=8, ctot=56),
           _c('halo32_c32_136', 'fwd', 1, 9, 33, 32, 0, 136, 32, bias=True, res=True, act=R, ldr=140, stat=True, split=False),
           _c('halo32_cat_c40', 'fwd', 2, 5, 17, 16, 48, 40, 32, ld1=20, ld2=52, act=L, ldo=44),
           _c('halo32_bn', 'fwd', 1, 10, 35, 32, 0, 72, 32, bias=True, bnpart=True),
           _c('halo32_dgrad_slice', 'dgrad', 1, 6, 40, 48, 0, 34, 32, c_lo=20, ctot=60, ldo=40),
           _c('halo30_c16_264', 'fwd', 1, 127, 225, 16, 0, 264, 30, bias=True, act=R, k32=0),
           _c('halo30_bn', 'fwd', 1, 127, 225, 16, 0, 258, 30, bnpart=True, ldo=264, k32=0),
           _c('halo31_c144_34', 'fwd', 2, 127, 500, 144, 0, 34, 31, res=True, act=L, ldo=40),
           _c('halo31_bn', 'fwd', 2, 127, 500, 144, 0, 36, 31, bias=True, bnpart=True)]
    # ---- halo split-K (+ conv_splitk_reduce_kernel): slab counts that do not divide the chunk count (11 chunks in 2 slabs of 6 + 5,
    # 13 in 3 of 5 + 5 + 3), the halo16 tiles, and the Cout 17..32 path of uses_dma (17 chunks in 4 slabs of 5 + 5 + 5 + 2)
    cs += [_c('splitk32_c176_40', 'fwd', 1, 9, 33, 176, 0, 40, 32, ws=2, bias=True, res=True, act=R, ldo=44, stat=True),
           _c('splitk32_c208_136', 'fwd', 1, 5, 17, 128, 80, 134, 32, ws=3, act=L, bias=True, ldo=140),
           _c('splitk34_c208_40', 'fwd', 2, 9, 12, 208, 0, 40, 34, ws=3, res=True),
           _c('splitk33_dgrad', 'dgrad', 1, 9, 16, 176, 0, 132, 33, ws=2, ctot=132),
           _c('splitk32_c272_24', 'fwd', 1, 9, 33, 272, 0, 24, 32, ws=4, bias=True, act=R, stat=True),
           _c('splitk32_c272_22_dgrad', 'dgrad', 1, 7, 20, 272, 0, 22, 32, ws=4, ctot=22, res=True)]
    # ---- halo_x3 (40 / 41: the fp32 ids 30 / 32 with w_split, Cout % 128 / % 64 == 0, k32 mode 0) and the merged parity classes (42)
    cs += [_c('x3_41_c32_64', 'fwd', 1, 9, 33, 32, 0, 64, 41, fmt=64, k32=0, bias=True, res=True, act=R, ldr=68, stat=True),
           _c('x3_41_cat_192', 'fwd', 2, 5, 17, 16, 48, 192, 41, fmt=64, k32=0, ld1=20, ld2=52, act=L, ldo=196, stat=True),
           _c('x3_41_bn', 'fwd', 1, 10, 35, 32, 0, 128, 41, fmt=64, k32=0, bias=True, bnpart=True),
           _c('x3_41_dgrad_slice', 'dgrad', 1, 6, 40, 48, 0, 64, 41, fmt=64, k32=0, c_lo=64, ctot=192),
           _c('x3_40_c16_256', 'fwd', 1, 190, 250, 16, 0, 256, 40, fmt=128, k32=0, bias=True, act=R),
           _c('x3_40_bn', 'fwd', 1, 190, 250, 16, 0, 256, 40, fmt=128, k32=0, bnpart=True, ldo=260),
           _c('parity_c16_64', 'dgrad', 2, 21, 35, 16, 0, 64, 42, fmt=64, stride=2, cls='merge', stat=True),
           _c('parity_slice_ld', 'dgrad', 1, 11, 77, 32, 0, 64, 42, fmt=64, stride=2, cls='merge', c_lo=64, ctot=192, ld1=36, ldo=68, act=L),
           _c('parity_even', 'dgrad', 1, 8, 34, 16, 0, 128, 42, fmt=64, stride=2, cls='merge', act=R)]
    # ---- dma_x3 (50 / 51: >= 4096 grid pixels, Cout % 64 / % 128 == 0).  The split-once body (ssg_conv_dma_body 2) has its own file
    # (tests/test_conv_dma_split_once_gpu.py: partial tiles, straddling chunks, row slices, stride 2, odd step counts); here one case of
    # it per id through the C-ABI, and the older body (1), which runs where a pixel stride is no multiple of 4
    cs += [_c('dmax3_50_new', 'fwd', 1, 72, 60, 48, 16, 64, 50, fmt=64, body=2, k=1, bias=True, res=True, act=R, stat=True),
           _c('dmax3_51_new_s2', 'fwd', 1, 132, 126, 32, 0, 128, 51, fmt=128, body=2, stride=2, act=L, bias=True),
           _c('dmax3_50_cls_slice', 'dgrad', 1, 131, 127, 32, 0, 64, 50, fmt=64, body=2, stride=2, cls=(1, 0), c_lo=64, ctot=192, ld1=36),
           _c('dmax3_50_bn', 'fwd', 1, 72, 60, 32, 0, 64, 50, fmt=64, body=2, k=1, bias=True, bnpart=True),
           _c('dmax3_51_cat', 'fwd', 1, 72, 60, 48, 16, 128, 51, fmt=128, body=2, k=1, ld1=52, res=True, act=R, ldr=132),
           _c('dmax3_50_old', 'fwd', 1, 72, 60, 48, 0, 64, 50, fmt=64, body=1, k=1, bias=True, res=True, act=R, ldo=65, ldr=68, stat=True),
           _c('dmax3_50_old_cat_s2', 'fwd', 1, 131, 127, 16, 32, 64, 50, fmt=64, body=1, stride=2, ld2=36, ldo=67, act=L),
           _c('dmax3_51_old_bn', 'fwd', 1, 72, 60, 32, 0, 128, 51, fmt=128, body=1, k=1, bias=True, bnpart=True, ldo=129),
           _c('dmax3_51_old_cls', 'dgrad', 1, 131, 127, 32, 0, 128, 51, fmt=128, body=1, stride=2, cls=(0, 1), c_lo=128, ctot=256, ldo=131, stat=True)]
    # ---- k32 (60..64), ssg_conv_set_k32_mode(2): formats 1128 (Cout % 128 == 0), 2064 (Cout % 64 == 0, GH % 16 == 0, no in_scale),
    # 1064 (else), 1016 / 1032 (Cout 12..16 / 17..32 with Cin >= 128); GW = 17 and 33, GH no tile multiple (except 2064), one
    # 32-channel chunk and several, concat, fused input transform (60 / 61) and backward statistics (60 / 61 / 62) with each activation
    cs += [_c('k32_60_w33', 'fwd', 2, 11, 33, 32, 0, 128, 60, fmt=1128, k32=2, bias=True, res=True, act=R, ldr=132, stat=True),
           _c('k32_60_w17_cat', 'fwd', 1, 9, 17, 32, 64, 256, 60, fmt=1128, k32=2, ld1=36, ld2=68, ldo=260, act=L),
           _c('k32_60_bn', 'fwd', 1, 19, 40, 64, 0, 128, 60, fmt=1128, k32=2, bias=True, bnpart=True),
           _c('k32_60_dgrad_slice', 'dgrad', 1, 10, 35, 64, 0, 128, 60, fmt=1128, k32=2, c_lo=128, ctot=384, res=True),
           _c('k32_60_aff_none', 'fwd', 1, 11, 33, 64, 0, 128, 60, fmt=1128, k32=2, aff=ACT_NONE, bias=True),
           _c('k32_60_aff_relu', 'fwd', 2, 11, 33, 32, 0, 128, 60, fmt=1128, k32=2, aff=R, act=R, stat=True),
           _c('k32_60_aff_lrelu', 'fwd', 1, 9, 17, 64, 0, 128, 60, fmt=1128, k32=2, aff=L, ld1=68, bnpart=True),
           _c('k32_60_bwd_relu', 'dgrad', 2, 11, 33, 32, 0, 128, 60, fmt=1128, k32=2, bwd=R, stat=True),
           _c('k32_60_bwd_lrelu', 'dgrad', 1, 9, 17, 64, 0, 128, 60, fmt=1128, k32=2, bwd=L, ldr=132, ldo=132),
           _c('k32_60_bwd_none', 'dgrad', 1, 5, 20, 32, 0, 128, 60, fmt=1128, k32=2, bwd=ACT_NONE),
           _c('k32_61_w33', 'fwd', 2, 11, 33, 32, 0, 64, 61, fmt=1064, k32=2, bias=True, res=True, act=R, ldr=68, stat=True),
           _c('k32_61_w17_cat', 'fwd', 1, 9, 17, 64, 32, 192, 61, fmt=1064, k32=2, ld2=36, ldo=196, act=L),
           _c('k32_61_bn', 'fwd', 1, 19, 40, 64, 0, 64, 61, fmt=1064, k32=2, bias=True, bnpart=True),
           _c('k32_61_dgrad_slice', 'dgrad', 1, 10, 35, 64, 0, 64, 61, fmt=1064, k32=2, c_lo=64, ctot=192),
           _c('k32_61_aff_none', 'fwd', 1, 16, 33, 32, 0, 64, 61, fmt=1064, k32=2, aff=ACT_NONE),
           _c('k32_61_aff_relu', 'fwd', 2, 11, 33, 32, 0, 64, 61, fmt=1064, k32=2, aff=R, bias=True, stat=True),
           _c('k32_61_aff_lrelu', 'fwd', 1, 9, 17, 64, 0, 64, 61, fmt=1064, k32=2, aff=L, res=True, act=L, ld1=68),
           _c('k32_61_bwd_relu', 'dgrad', 2, 11, 33, 32, 0, 64, 61, fmt=1064, k32=2, bwd=R, stat=True),
           _c('k32_61_bwd_lrelu', 'dgrad', 1, 9, 17, 64, 0, 64, 61, fmt=1064, k32=2, bwd=L),
           _c('k32_61_bwd_none', 'dgrad', 1, 5, 20, 32, 0, 64, 61, fmt=1064, k32=2, bwd=ACT_NONE),
           _c('k32_62_w33', 'fwd', 1, 16, 33, 32, 0, 64, 62, fmt=1064, k32=2, bias=True, res=True, act=R, ldr=72, stat=True),
           _c('k32_62_w17_cat', 'fwd', 1, 32, 17, 32, 64, 192, 62, fmt=1064, k32=2, ld1=36, act=L, ldo=200),
           _c('k32_62_bn', 'fwd', 2, 16, 40, 64, 0, 64, 62, fmt=1064, k32=2, bias=True, bnpart=True),
           _c('k32_62_dgrad_slice', 'dgrad', 1, 16, 35, 64, 0, 64, 62, fmt=1064, k32=2, c_lo=64, ctot=192),
           _c('k32_62_bwd_relu', 'dgrad', 1, 16, 33, 32, 0, 64, 62, fmt=1064, k32=2, bwd=R, stat=True),
           _c('k32_62_bwd_lrelu', 'dgrad', 1, 32, 17, 64, 0, 64, 62, fmt=1064, k32=2, bwd=L),
           _c('k32_62_bwd_none', 'dgrad', 1, 16, 20, 32, 0, 64, 62, fmt=1064, k32=2, bwd=ACT_NONE),
           _c('k32_63_c128_16', 'fwd', 2, 11, 33, 128, 0, 16, 63, fmt=1016, k32=2, bias=True, res=True, act=R, stat=True),
           _c('k32_63_cat_12', 'fwd', 1, 9, 17, 64, 96, 12, 63, fmt=1016, k32=2, ld2=100, act=L, ldo=16),
           _c('k32_63_bn', 'fwd', 1, 19, 40, 128, 0, 16, 63, fmt=1016, k32=2, bnpart=True),
           _c('k32_63_dgrad_slice', 'dgrad', 1, 9, 17, 128, 0, 16, 63, fmt=1016, k32=2, c_lo=4, ctot=24, ld1=132, res=True, ldr=20),
           _c('k32_64_cat', 'fwd', 1, 9, 17, 64, 64, 28, 64, fmt=1032, k32=2, ld1=68, res=True, ldo=32, ldr=36),
           _c('k32_64_c128_32', 'fwd', 2, 11, 33, 128, 0, 32, 64, fmt=1032, k32=2, bias=True, res=True, act=R, stat=True),
           _c('k32_64_dgrad_20', 'dgrad', 1, 9, 17, 160, 0, 20, 64, fmt=1032, k32=2, c_lo=4, ctot=28, ldo=24),
           _c('k32_64_bn', 'fwd', 1, 19, 40, 128, 0, 24, 64, fmt=1032, k32=2, bias=True, bnpart=True)]
    # ... and in the default mode 1, where the smallest grid that fills the chip stays small: 1128 at 256 workgroups of 8 x 32 pixels,
    # 1016 / 1032 at 192.  (61 needs 1536 workgroups of 4 x 32 pixels and 62 2048 of 16 x 32, both at Cout = 64 exactly -- a wider
    # Cout is the <128,128> tile's, whose split form wants Cout % 128 == 0 -- so 196 608 and 1 048 576 pixels: mode 1 differs from
    # mode 2 only in the host predicate, which tests/test_conv_plan.py pins.)
    cs += [_c('k32_60_mode1', 'fwd', 1, 128, 512, 32, 0, 128, 60, fmt=1128, bias=True, act=R),
           _c('k32_63_mode1', 'fwd', 1, 96, 512, 128, 0, 16, 63, fmt=1016, res=True),
           _c('k32_64_mode1', 'fwd', 1, 96, 512, 128, 0, 20, 64, fmt=1032, act=L, bias=True)]
    # ---- ssg_conv2d_igemm_f32 (the MFMA path alone) at a thin shape: ssg_conv2d_kernel_id describes ssg_conv2d_f32's dispatch (the thin
    # kernel, id 10); this entry point runs the register-staged kernel on the same descriptor
    cs += [_c('igemm_thin_shape', 'fwd', 2, 9, 19, 24, 0, 3, 10, bias=True, act=L, entry='igemm', stat=True)]
    return cs


CASES = _cases()
NONFINITE_CASES = ['x3_40_c16_256', 'x3_41_c32_64', 'parity_c16_64', 'k32_60_w33', 'k32_61_w33', 'k32_62_w33', 'k32_63_c128_16', 'k32_64_c128_32']


def case(name):
    return next(c for c in CASES if c.name == name)


# ============================================================================ 10. coverage
def facts(c):
    """What a case exercises, from its geometry."""
    g = geom(c)
    f = set()
    chunk = 32 if (c.kid in K32_IDS or c.body == 2) else 16
    if c.C2:
        f.add('concat')
        if c.C1 % chunk:
            f.add('straddle')                                   # a K-step chunk that holds channels of both inputs
        if g.ld2 != g.ld1:
            f.add('ld2!=ld1')
    f |= {n for n, on in (('bias', c.bias), ('res', c.res), ('relu', c.act == ACT_RELU), ('lrelu', c.act == ACT_LRELU)) if on}
    if c.Cout % 4:
        f.add('cout%4')
    if c.kid in COL_TILE and c.Cout % COL_TILE[c.kid]:
        f.add('cout_tile')
    if c.kid in OUT_TILE:
        th, tw = OUT_TILE[c.kid]
        for _, _, GHq, GWq, _ in g.groups:
            if GWq % tw and GWq > tw:
                f.add('ragged_x')
            if GHq % th and GHq > th:
                f.add('ragged_y')
            if GWq < tw:
                f.add('narrow')
    if g.ld1 > c.C1:
        f.add('ld_in')
    if g.ldo > pad4(c.Cout):
        f.add('ld_out')
    if c.res and g.ldr > pad4(c.Cout) and g.ldr != g.ldo:
        f.add('ld_res')
    if c.op == 'dgrad':
        f.add('dgrad')
        if c.c_lo:
            f.add('slice')
    if g.cred_real < g.Cin:
        f.add('pad_channels')
    if c.stride == 2:
        f.add('stride2')
        if c.H % 2 or c.W % 2:
            f.add('s2_odd')
        if c.cls is not None and c.cls != 'merge':
            f.add('class')
    if c.k == 1:
        f.add('1x1')
    if g.kmode == 0 and len(k_steps(c, g, g.groups[0][4])) % 2:
        f.add('odd_steps')
    if g.kmode == 0 and g.Cin > chunk:
        f.add('chunks')
    if c.bnpart:
        f.add('bnpart')
    if c.ws:
        f.add('splitk')
    if c.aff is not None:
        f.add('aff%d' % c.aff)
    if c.bwd is not None:
        f.add('bwd%d' % c.bwd)
    if c.k32 == 1 and c.kid in K32_IDS:
        f.add('mode1')
    if c.stat:
        f.add('stat')
    return f


# What each route ACCEPTS, written from the host predicates (validate / plan_conv in conv_igemm.hip and the family predicates it calls),
# not from the table.  Every descriptor may carry bias, res, either activation and pixel strides wider than the channels on every
# tensor; `stat` = class (b)'s companion, the RMS gate against the emulation.
_EPI = {'bias', 'res', 'relu', 'lrelu', 'ld_in', 'ld_out', 'ld_res', 'stat'}
_TWO = {'concat', 'ld2!=ld1'}                                   # a second input pointer with its own pixel stride
_DG = {'dgrad', 'slice'}                                        # mirrored taps; desc.w offset by row0 Kp into a transposed pack
_ANY = {'stride2', 's2_odd', 'class', '1x1'}                    # any tap list and strides (validate): not the 3x3 unit-stride window only
_TILE = {'ragged_x', 'ragged_y', 'narrow'}
_COUT = {'cout%4', 'cout_tile'}                                 # any Cout: pad lanes, a partial column tile
_K0 = {'chunks', 'odd_steps'}                                   # kmode 0 K loop: several chunks, an odd K-step count (ring stage parity)
_HALO = _EPI | _TWO | _DG | _TILE | _K0 | {'bnpart'}
ACCEPTS = {
    # register-staged: whatever validate() passes that no other family takes (kmode 1, or Cout <= 32); no statistics, no split-K
    0: _EPI | _TWO | _DG | _ANY | _TILE | _COUT | {'pad_channels'},
    1: _EPI | _TWO | _DG | _ANY | _TILE | _COUT | {'pad_channels'},
    2: _EPI | _TWO | _DG | _ANY | _TILE | _COUT | {'pad_channels'},
    # ssg_thin_conv_kind / ssg_thin4_conv_kind: one input, unit strides, the whole image
    10: _EPI | _DG | {'cout%4', '1x1', 'pad_channels'},
    12: _EPI | _DG | {'cout%4', '1x1', 'pad_channels'},
    13: _EPI | _DG | {'cout%4'},
    14: _EPI | _DG | {'cout%4', 'pad_channels'},
    15: _EPI | _DG | {'cout%4', 'pad_channels'},
    16: _EPI | {'cout%4', '1x1'},                               # ssg_conv1x1_k64_ok: the plain 1x1 tap of 64 channels, no bnpart
    # uses_dma && !uses_halo: kmode 0, Cout > 32
    20: _EPI | _TWO | _DG | _ANY | _TILE | _COUT | _K0 | {'bnpart'},
    21: _EPI | _TWO | _DG | _ANY | _TILE | _COUT | _K0 | {'bnpart'},
    22: _EPI | _TWO | _DG | _ANY | _TILE | _COUT | {'bnpart'},
    # ssg_conv_halo_ok: the nine taps of the 3x3 window at unit stride, kmode 0; split-K on variants 2..4 (ssg_conv_halo_ksplit)
    30: _HALO | _COUT, 31: _HALO | _COUT, 32: _HALO | _COUT | {'splitk'}, 33: _HALO | _COUT | {'splitk'}, 34: _HALO | _COUT | {'splitk'},
    # ssg_conv_halo_x3_ok: whole column tiles; ssg_conv_halo_x3_parity_ok: the merged stride-2 gradient, no bias / res / bnpart
    40: _HALO, 41: _HALO,
    42: {'relu', 'lrelu', 'ld_in', 'ld_out', 'stat', 'dgrad', 'slice', 'stride2', 's2_odd', 'chunks'} | _TILE,
    # ssg_conv_dma_x3_bn: the LDS-DMA family on whole 64- / 128-column tiles, >= 4096 grid pixels
    50: _EPI | _TWO | _DG | _ANY | {'ragged_x', 'ragged_y', 'bnpart', 'straddle'},
    51: _EPI | _TWO | _DG | _ANY | {'ragged_x', 'ragged_y', 'bnpart', 'straddle'},
    # ssg_conv_halo_k32_fmt: 32-channel multiples on both inputs, GW >= 17; in_scale on <8,128> / <4,64>, bwd_x on the three wide tiles
    60: _HALO | {'aff0', 'aff1', 'aff2', 'bwd0', 'bwd1', 'bwd2', 'mode1'},
    61: _HALO | {'aff0', 'aff1', 'aff2', 'bwd0', 'bwd1', 'bwd2', 'mode1'},
    62: _HALO | {'bwd0', 'bwd1', 'bwd2', 'mode1'},
    63: _HALO | {'mode1'}, 64: _HALO | {'mode1'},
}
_LARGE = ('the smallest grid of this route holds 28 000 - 130 000 pixels: its two or three cases carry what they can, the rest runs on the '
          'small sibling that shares the code (thin4 / LDS-DMA for 15 / 16, id 32 for 30 / 31, id 41 for 40)')
_NO_EMUL = 'the float32 emulation of a 28 000 - 130 000-pixel case takes minutes: class (b) runs there as at every case, the RMS gate does not'
# accepted features the table leaves out on purpose, each with its reason
EXEMPT = {
    0: {}, 1: {}, 2: {}, 10: {}, 12: {}, 13: {}, 14: {},
    15: dict({f: _LARGE for f in ('lrelu', 'slice', 'cout%4')}, stat=_NO_EMUL),
    16: dict({f: _LARGE for f in ('ld_res',)}, stat=_NO_EMUL),
    20: {'narrow': 'a stride-2 or 1x1 grid narrower than 16 pixels with Kp > 256 is the tile map of id 22, which has it'},
    21: {'narrow': 'as id 20'},
    22: {},
    30: dict({f: _LARGE for f in ('res', 'lrelu', 'ld_in', 'ld_res', 'concat', 'ld2!=ld1', 'dgrad', 'slice', 'narrow', 'chunks')}, stat=_NO_EMUL),
    31: dict({f: _LARGE for f in ('relu', 'ld_in', 'ld_res', 'concat', 'ld2!=ld1', 'dgrad', 'slice', 'narrow')}, stat=_NO_EMUL),
    32: {}, 33: {'ragged_x': 'halo16 is chosen for GW <= 16 = one tile', 'odd_steps': 'covered with chunks by id 34, the same body'},
    34: {'ragged_x': 'as id 33'},
    40: dict({f: _LARGE for f in ('res', 'lrelu', 'ld_in', 'ld_res', 'concat', 'ld2!=ld1', 'dgrad', 'slice', 'narrow', 'chunks')}, stat=_NO_EMUL),
    41: {}, 42: {'ragged_y': None},
    50: {}, 51: {},
    60: {}, 61: {'mode1': 'needs 196 608 pixels at Cout = 64 (see the case table)'},
    62: {'mode1': 'needs 1 048 576 pixels (see the case table)', 'ragged_y': 'mode 2 gives the 16-row tile only where GH % 16 == 0'},
    63: {}, 64: {},
}
del EXEMPT[42]['ragged_y']


def check_coverage():
    """Every reachable kernel id appears, with every feature the route accepts (ACCEPTS) but those EXEMPT names with a reason -- `stat`
    (class (b)'s RMS companion) among them, so every id but the five large-grid ones has a stat case; class (b) itself runs at every
    case; both LDS-DMA split bodies; the igemm entry point; every parity class as a launch of its own.  Returns {id: set of facts}."""
    hit, names, bodies, entries = {}, set(), set(), set()
    for c in CASES:
        assert c.name not in names, c.name
        names.add(c.name)
        g = geom(c)
        assert g.GH >= 1 and g.GW >= 1 and c.C1 % 4 == 0 and c.C2 % 4 == 0 and g.ldo >= c.Cout, c.name
        assert (g.GH - 1) * g.out_s + g.oy < g.OH and (g.GW - 1) * g.out_s + g.ox < g.OW, c.name
        assert c.kid in REACHABLE_IDS, (c.name, c.kid)
        assert not (c.bnpart and (c.res or c.act)), '%s: the rows are judged against the output, which must be acc + bias' % c.name
        assert not (c.bwd is not None and (c.bias or c.res or c.act or c.aff is not None)), c.name
        hit.setdefault(c.kid, set()).update(facts(c))
        if c.body:
            bodies.add((c.kid, c.body))
        entries.add(c.entry)
    for kid in REACHABLE_IDS:
        assert kid in hit, 'no case reaches kernel id %d' % kid
        assert set(EXEMPT[kid]) <= ACCEPTS[kid] and all(EXEMPT[kid].values()), kid
        need = ACCEPTS[kid] - set(EXEMPT[kid])
        assert need <= hit[kid], 'kernel id %d: no case with %s' % (kid, sorted(need - hit[kid]))
    assert bodies == {(50, 1), (50, 2), (51, 1), (51, 2)}, bodies
    assert entries == {'f32', 'igemm'}
    assert {c.cls for c in CASES if c.cls not in (None, 'merge')} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    for n in NONFINITE_CASES:
        assert case(n).kid in SPLIT_IDS
    assert {case(n).kid for n in NONFINITE_CASES} == {40, 41, 42, 60, 61, 62, 63, 64}
    return hit
