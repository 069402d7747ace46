"""Training augmentation on the device: the reference's albumentations pipeline -- Rotate, Flip,
HueSaturationValue(10, 10, 10), RandomBrightnessContrast(0.1, 0.1), Resize, Normalize (train_seg_gan.py:366-377,
train.py:339-349) -- drawn on the host per sample and applied by one HIP launch per batch (`ops.augment_batch`).

The host side is pure numpy: `sample_params` draws from a seeded `numpy.random.Generator` in a fixed order and encodes each
sample as one int32 row and one 256-byte table; `DeviceAugment` is the callable a trainer finds under
config['device_augment'].  The arithmetic of the transform itself is defined by tests/augment_ref.py.
"""
import math

import numpy as np
import torch

from . import ops

ROW = ops.AUG_ROW
FLAG_HSV = 1
ONE = 1 << 16

# Flip() draws d in {-1, 0, 1} as cv2.flip takes it: 0 = vertical (rows reversed), 1 = horizontal, -1 = both
FLIP_NONE, FLIP_H, FLIP_V, FLIP_BOTH = 0, 1, 2, 3
_FLIP_OF_D = {1: FLIP_H, 0: FLIP_V, -1: FLIP_BOTH}

DRAW_DTYPE = np.dtype([('rotate', '?'), ('angle', 'f8'), ('flip', 'i4'), ('hsv', '?'), ('dh', 'i4'), ('ds', 'i4'), ('dv', 'i4'),
                       ('bc', '?'), ('alpha', 'f8'), ('beta', 'f8')])


def affine_fp64(src_hw, out_hw, angle_deg=0.0, flip=FLIP_NONE):
    """The inverse map of Rotate . Flip . Resize in fp64, as a 2 x 3 matrix A: output pixel (i, j) (row, column) reads the source
    at pixel-index coordinates (sx, sy) = A @ (j, i, 1).  Right to left: output pixel centre (j + 1/2, i + 1/2); scale src / out
    per axis (Resize); mirror about the source (Flip); rotate about the source centre by the drawn angle, counter-clockwise
    positive as cv2.getRotationMatrix2D (Rotate); back to pixel indices (- 1/2)."""
    h, w = float(src_hw[0]), float(src_hw[1])
    oh, ow = float(out_hw[0]), float(out_hw[1])
    centre_out = np.array([[1, 0, 0.5], [0, 1, 0.5], [0, 0, 1]], dtype=np.float64)
    scale = np.array([[w / ow, 0, 0], [0, h / oh, 0], [0, 0, 1]], dtype=np.float64)
    fl = np.eye(3, dtype=np.float64)
    if flip in (FLIP_H, FLIP_BOTH):
        fl[0, 0], fl[0, 2] = -1.0, w
    if flip in (FLIP_V, FLIP_BOTH):
        fl[1, 1], fl[1, 2] = -1.0, h
    a = math.radians(float(angle_deg))
    ca, sa = math.cos(a), math.sin(a)
    cx, cy = w / 2.0, h / 2.0
    rot = np.array([[ca, -sa, cx - ca * cx + sa * cy], [sa, ca, cy - sa * cx - ca * cy], [0, 0, 1]], dtype=np.float64)
    centre_src = np.array([[1, 0, -0.5], [0, 1, -0.5], [0, 0, 1]], dtype=np.float64)
    return (centre_src @ rot @ fl @ scale @ centre_out)[:2]


def fixed_map(a):
    """The six 16.16 entries m0 .. m5 of a 2 x 3 fp64 map, each rounded to nearest."""
    m = np.rint(np.asarray(a, dtype=np.float64).reshape(6) * ONE)
    if not (np.abs(m) < 2.0 ** 31).all():
        raise ValueError('augment: the map %s does not fit 16.16 fixed point in int32' % (a,))
    return m.astype(np.int32)


def bc_lut(alpha, beta):
    """albumentations' uint8 table of RandomBrightnessContrast(brightness_by_max=True)."""
    lut = np.arange(256, dtype=np.float32)
    lut = lut * np.float32(alpha)
    lut = lut + np.float32(beta * 255)
    return np.clip(lut, 0, 255).astype(np.uint8)


def draw_params(n, config, generator, hue_shift_limit=10, sat_shift_limit=10, val_shift_limit=10,
                brightness_limit=0.1, contrast_limit=0.1):
    """The raw draws of n samples as a record array (DRAW_DTYPE).  Per sample, in this order and whatever the outcomes -- so the
    position in the generator's stream depends on n alone:
      1. random() < 0.5: Rotate applies;       2. uniform(rotate_min, rotate_max): its angle in degrees;
      3. random() < 0.5: Flip applies;         4. integers(-1, 2): its code d (0 vertical, 1 horizontal, -1 both);
      5. random() < 0.5: the HSV stage applies; 6 - 8. integers(-limit, limit + 1): dh, ds, dv;
      9. random() < 0.5: brightness / contrast applies; 10. uniform(-contrast_limit, contrast_limit): alpha - 1;
      11. uniform(-brightness_limit, brightness_limit): beta.
    Every stage has albumentations' default p = 0.5."""
    lo, hi = float(config['rotate_min']), float(config['rotate_max'])
    d = np.zeros(n, dtype=DRAW_DTYPE)
    for k in range(n):
        d['rotate'][k] = generator.random() < 0.5
        d['angle'][k] = generator.uniform(lo, hi)
        flip_on = generator.random() < 0.5
        code = int(generator.integers(-1, 2))
        d['flip'][k] = _FLIP_OF_D[code] if flip_on else FLIP_NONE
        d['hsv'][k] = generator.random() < 0.5
        d['dh'][k] = generator.integers(-hue_shift_limit, hue_shift_limit + 1)
        d['ds'][k] = generator.integers(-sat_shift_limit, sat_shift_limit + 1)
        d['dv'][k] = generator.integers(-val_shift_limit, val_shift_limit + 1)
        d['bc'][k] = generator.random() < 0.5
        d['alpha'][k] = 1.0 + generator.uniform(-contrast_limit, contrast_limit)
        d['beta'][k] = generator.uniform(-brightness_limit, brightness_limit)
    return d


def encode_params(draws, src_hw, out_hw):
    """(int32 [n, 16] rows, uint8 [n, 256] tables) of a `draw_params` record array."""
    n = len(draws)
    params = np.zeros((n, ROW), dtype=np.int32)
    luts = np.empty((n, 256), dtype=np.uint8)
    for k in range(n):
        d = draws[k]
        params[k, :6] = fixed_map(affine_fp64(src_hw, out_hw, d['angle'] if d['rotate'] else 0.0, int(d['flip'])))
        if d['hsv']:
            params[k, 6:10] = (FLAG_HSV, d['dh'], d['ds'], d['dv'])
        luts[k] = bc_lut(d['alpha'], d['beta']) if d['bc'] else np.arange(256, dtype=np.uint8)
    return params, luts


def sample_params(n, src_hw, out_hw, config, generator, **limits):
    """Draw the augmentation of n samples of src_hw = (H, W) tiles resampled to out_hw: (params int32 [n, 16], luts uint8 [n, 256])
    for `ops.augment_batch`.  Host code only; a generator in the same state gives the same tables (`draw_params` documents the
    order).  config supplies rotate_min / rotate_max in degrees; the other limits are the reference's literals, overridable by
    keyword: hue_shift_limit, sat_shift_limit, val_shift_limit (10), brightness_limit, contrast_limit (0.1)."""
    return encode_params(draw_params(n, config, generator, **limits), src_hw, out_hw)


def plain_params(n, src_hw, out_hw):
    """The reference's val_transform: the scale map alone, no colour stage."""
    params = np.zeros((n, ROW), dtype=np.int32)
    params[:, :6] = fixed_map(affine_fp64(src_hw, out_hw))
    luts = np.tile(np.arange(256, dtype=np.uint8), (n, 1))
    return params, luts


def _as_bytes(x, channels_ok, what, top):
    """uint8 [N, H, W, C] on the device from either accepted form."""
    if x.dtype == torch.uint8:
        if x.dim() != 4 or not channels_ok(x.shape[3]):
            raise TypeError('DeviceAugment: expected uint8 [N, H, W, C] %s, got %s' % (what, tuple(x.shape)))
        return x
    if x.dtype != torch.float32 or x.dim() != 4 or not channels_ok(x.shape[1]):
        raise TypeError('DeviceAugment: expected %s as uint8 [N, H, W, C] or float32 [N, C, H, W], got %s %s' % (what, x.dtype, tuple(x.shape)))
    if not bool(((x == x.round()) & (x >= 0) & (x <= top)).all()):
        raise ValueError('DeviceAugment: float32 %s must hold integers in 0 .. %d (the reference\'s Dataset(transform=None))' % (what, top))
    return x.permute(0, 2, 3, 1).to(torch.uint8).contiguous()


class DeviceAugment(object):
    """`(images, masks) -> (input, target)` on the device, for config['device_augment'] of the trainers.

    images / masks: uint8 [N, H, W, 3] (B, G, R as cv2.imread gives them) and [N, H, W, C], or what the reference's
    Dataset(transform=None) collates: float32 [N, 3, H, W] holding integers 0 .. 255 and float32 [N, C, H, W] holding 0 / 1
    (anything else raises ValueError); these are converted to bytes with torch ops on the device.  The output size is
    config['input_h'] x config['input_w'].  train=True draws the reference's train_transform per sample from
    numpy.random.default_rng(SeedSequence(seed, spawn_key=(rank,))): one (seed, rank) reproduces a run, data-parallel ranks draw
    different parameters; train=False is its val_transform (scale map and Normalize only, nothing drawn)."""

    def __init__(self, config, seed=0, train=True, rank=0, border=(0, 0, 0), **limits):
        self.config = dict(rotate_min=config['rotate_min'], rotate_max=config['rotate_max']) if train else {}
        self.out_hw = (int(config['input_h']), int(config['input_w']))
        self.train = bool(train)
        self.border = tuple(border)
        self.limits = limits
        self.generator = np.random.default_rng(np.random.SeedSequence(int(seed), spawn_key=(int(rank),)))
        self._validation = None

    def validation(self):
        """The train=False twin (same output size and border), which validate() of the trainers applies: itself if it is one."""
        if not self.train:
            return self
        if self._validation is None:
            self._validation = DeviceAugment(dict(input_h=self.out_hw[0], input_w=self.out_hw[1]), train=False, border=self.border)
        return self._validation

    def __call__(self, images, masks):
        img = _as_bytes(images, lambda c: c == 3, 'images', 255)
        msk = _as_bytes(masks, lambda c: 1 <= c <= 8, 'masks', 1)
        n, src_hw = img.shape[0], (img.shape[1], img.shape[2])
        if self.train:
            params, luts = sample_params(n, src_hw, self.out_hw, self.config, self.generator, **self.limits)
        else:
            params, luts = plain_params(n, src_hw, self.out_hw)
        return ops.augment_batch(img, msk, params, luts, self.out_hw[0], self.out_hw[1], border=self.border)
