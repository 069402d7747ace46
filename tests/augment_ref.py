"""The training augmentation of ssunet_gan_amd.augment / csrc/augment.hip, stated in numpy: one operation per statement,
integer dtypes wherever the definition is in integers.  This module is the definition; the kernel implements
exactly this and the GPU tests compare byte for byte.

A sample is described by a row of 16 int32 and a 256-byte table:
  row[0:6]  m0 .. m5, 16.16 fixed point: output pixel (i, j) (row, column) reads the source at
            sx = m0 * j + m1 * i + m2,  sy = m3 * j + m4 * i + m5   (int64; pixel-index coordinates, half-pixel shifts folded in)
  row[6]    flags: bit 0 = apply the hue / saturation / value stage; every other bit must be 0
  row[7:10] dh, ds, dv: the integer shifts of that stage (|dh| <= 179, |ds|, |dv| <= 255)
  row[10:]  0
  lut       the brightness / contrast table, indexed with the byte after the HSV stage (identity: stage not drawn)
"""
import numpy as np

ROW = 16
FLAG_HSV = 1


def norm_consts():
    """mean * 255 and 1 / (std * 255) of albumentations Normalize() in fp32: the expressions of ops._sw_norm_consts()."""
    mean = np.array((0.485, 0.456, 0.406), dtype=np.float32) * 255.0
    std = np.array((0.229, 0.224, 0.225), dtype=np.float32) * 255.0
    denom = np.reciprocal(std, dtype=np.float32)
    return mean.astype(np.float32), denom.astype(np.float32)


def pad4(c):
    return (c + 3) // 4 * 4


# ----------------------------------------------------------------------------- hue / saturation / value in integers
def hsv_from_bgr(b, g, r):
    """Integer arrays b, g, r in 0 .. 255 -> (H in 0 .. 179, S in 0 .. 255, V in 0 .. 255), every division rounded half up:
    V = max, S = 255 (V - min) / V, H = half the hue angle in degrees: 30 (g - b) / d, 60 + 30 (b - r) / d or
    120 + 30 (r - g) / d with d = V - min, by which of r, g, b (in that order of precedence) is the maximum; + 180 if negative."""
    b = b.astype(np.int32)
    g = g.astype(np.int32)
    r = r.astype(np.int32)
    v = np.maximum(np.maximum(b, g), r)
    mn = np.minimum(np.minimum(b, g), r)
    d = v - mn
    vs = np.maximum(v, 1)
    s = (510 * d + vs) // (2 * vs)
    is_r = v == r
    is_g = (~is_r) & (v == g)
    num = np.where(is_r, g - b, np.where(is_g, b - r, r - g))
    off = np.where(is_r, 0, np.where(is_g, 60, 120))
    ds = np.maximum(d, 1)
    h = (60 * num + ds) // (2 * ds)                      # floor((30 num / d) + 1 / 2): numpy's // floors
    h = h + off
    h = np.where(h < 0, h + 180, h)
    h = np.where(d == 0, 0, h)
    return h, s, v


def bgr_from_hsv(h, s, v):
    """The inverse on integers: sector = H // 30, f = H % 30, p = V (255 - S) / 255, q = V (7650 - S f) / 7650,
    t = V (7650 - S (30 - f)) / 7650, each rounded half up; (r, g, b) = (V, t, p), (q, V, p), (p, V, t), (p, q, V), (t, p, V),
    (V, p, q) for sectors 0 .. 5.  Returns (b, g, r)."""
    h = h.astype(np.int32)
    s = s.astype(np.int32)
    v = v.astype(np.int32)
    sec = h // 30
    f = h - 30 * sec
    p = (2 * v * (255 - s) + 255) // 510
    q = (2 * v * (7650 - s * f) + 7650) // 15300
    t = (2 * v * (7650 - s * (30 - f)) + 7650) // 15300
    r = np.choose(sec, [v, q, p, p, t, v])
    g = np.choose(sec, [t, v, v, q, p, p])
    b = np.choose(sec, [p, p, t, v, v, q])
    return b, g, r


def hsv_shift(b, g, r, dh, ds, dv):
    """H <- (H + dh) mod 180, S <- clip(S + ds, 0, 255), V <- clip(V + dv, 0, 255), and back to bytes."""
    h, s, v = hsv_from_bgr(b, g, r)
    h = np.mod(h + int(dh), 180)
    s = np.clip(s + int(ds), 0, 255)
    v = np.clip(v + int(dv), 0, 255)
    return bgr_from_hsv(h, s, v)


# ----------------------------------------------------------------------------- the whole transform
def check_row(row, out_h, out_w):
    """What the entry point refuses before it launches."""
    row = [int(x) for x in row]
    if row[6] & ~FLAG_HSV:
        raise ValueError('unknown flags %#x' % row[6])
    if abs(row[7]) > 179 or abs(row[8]) > 255 or abs(row[9]) > 255:
        raise ValueError('HSV shifts %s out of range' % (row[7:10],))
    for a, b_, c in (row[0:3], row[3:6]):
        if abs(a) * (out_w - 1) + abs(b_) * (out_h - 1) + abs(c) + (1 << 15) >= 1 << 62:
            raise ValueError('the map overflows int64')


def _taps(src, y, x, border):
    """src [H, W, K] uint8, integer index arrays y, x (int64) -> int64 [.., K]: the pixel, or `border` outside the source."""
    hh, ww = src.shape[0], src.shape[1]
    inside = (x >= 0) & (x < ww) & (y >= 0) & (y < hh)
    yc = np.where(inside, y, 0)
    xc = np.where(inside, x, 0)
    px = src[yc, xc].astype(np.int64)
    bd = np.asarray(border, dtype=np.int64).reshape((1,) * y.ndim + (-1,))
    return np.where(inside[..., None], px, bd)


def augment_one(img, mask, row, lut, out_h, out_w, border=(0, 0, 0)):
    """img [H, W, 3] uint8 (B, G, R), mask [H, W, C] uint8 -> (image float32 [out_h, out_w, 4],
    target float32 [out_h, out_w, pad4(C)]), pad lanes 0."""
    check_row(row, out_h, out_w)
    m = [np.int64(x) for x in row[:6]]
    i = np.arange(out_h, dtype=np.int64)[:, None]
    j = np.arange(out_w, dtype=np.int64)[None, :]
    sx = m[0] * j + m[1] * i + m[2]
    sy = m[3] * j + m[4] * i + m[5]
    # image: bilinear, 8-bit weights
    x0 = sx >> 16
    y0 = sy >> 16
    fx = ((sx >> 8) & 255)[..., None]
    fy = ((sy >> 8) & 255)[..., None]
    p00 = _taps(img, y0, x0, border)
    p01 = _taps(img, y0, x0 + 1, border)
    p10 = _taps(img, y0 + 1, x0, border)
    p11 = _taps(img, y0 + 1, x0 + 1, border)
    acc = (256 - fx) * (256 - fy) * p00
    acc = acc + fx * (256 - fy) * p01
    acc = acc + (256 - fx) * fy * p10
    acc = acc + fx * fy * p11
    px = (acc + (1 << 15)) >> 16
    b, g, r = px[..., 0], px[..., 1], px[..., 2]
    if int(row[6]) & FLAG_HSV:
        b, g, r = hsv_shift(b, g, r, row[7], row[8], row[9])
    lut = np.asarray(lut, dtype=np.uint8)
    mean, denom = norm_consts()
    out = np.zeros((out_h, out_w, 4), dtype=np.float32)
    for c, ch in enumerate((b, g, r)):
        byte = lut[ch]
        val = byte.astype(np.float32)
        val = val - mean[c]
        val = val * denom[c]
        out[..., c] = val
    # mask: nearest, border 0
    nx = (sx + (1 << 15)) >> 16
    ny = (sy + (1 << 15)) >> 16
    cm = mask.shape[2]
    mk = _taps(mask, ny, nx, (0,) * cm)
    tgt = np.zeros((out_h, out_w, pad4(cm)), dtype=np.float32)
    tgt[..., :cm] = mk.astype(np.float32)
    return out, tgt


def augment_ref(img, mask, params, luts, out_h, out_w, border=(0, 0, 0)):
    """img [N, H, W, 3] uint8, mask [N, H, W, C] uint8, params int32 [N, 16], luts uint8 [N, 256] ->
    (float32 [N, out_h, out_w, 4], float32 [N, out_h, out_w, pad4(C)]): the NHWC memory of the two tensors."""
    outs = [augment_one(img[n], mask[n], params[n], luts[n], out_h, out_w, border) for n in range(img.shape[0])]
    return np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs])
