"""CPU: the host side of the device augmentation (ssunet_gan_amd.augment) and its numpy definition (tests/augment_ref.py).

sample_params: reproducible, inside its ranges, tables as albumentations builds them, fixed-point map against the fp64
composition.  augment_ref: the cases whose answer is known without it (identity, flips, quarter turns, the 2 x 2 box).
HSV: the integer conversion against fp64 over all 2^24 colours, and the round-trip bound.

The round-trip bound (test_hsv_round_trip_bound).  With zero shifts the stage is bgr_from_hsv(hsv_from_bgr(.)).  V = max is exact,
so the largest channel comes back exactly.  Write d = max - min.  The stored S is 255 d / V rounded to an integer, so V S / 255
differs from d by at most V / 510 <= 1/2; the stored H is the hue in 2-degree steps rounded to an integer, off by at most 1/2 step.
Every channel is a continuous piecewise-linear function of the hue with slope at most (V S / 255) / 30 per step (one sector of 30
steps takes a channel from min to max), and a function of V S / 255 with slope at most 1.  Before its final rounding a
reconstructed channel is therefore within 1/2 + (1/2) (255 + 1/2) / 30 = 4.7583 of the original byte, and rounding a real number
within 4.7583 of an integer c to the nearest integer gives at most c + 5 or c - 5.  Bound: 5 per channel.  Measured maximum over
all 2^24 colours: 4."""
import numpy as np
import pytest

import augment_ref as ar

CONFIG = dict(rotate_min=-10, rotate_max=10, input_h=24, input_w=40)


@pytest.fixture(scope='module')
def aug(pkg):
    return pkg.augment


def _rows(aug, src_hw, out_hw, angle=0.0, flip=0, n=1):
    p = np.zeros((n, 16), dtype=np.int32)
    p[:, :6] = aug.fixed_map(aug.affine_fp64(src_hw, out_hw, angle, flip))
    return p, np.tile(np.arange(256, dtype=np.uint8), (n, 1))


def _source(h, w, c=3, seed=5):
    g = np.random.default_rng(seed)
    return g.integers(0, 256, (1, h, w, 3), dtype=np.uint8), g.integers(0, 2, (1, h, w, c), dtype=np.uint8)


def _normalized(img):
    mean, denom = ar.norm_consts()
    out = np.zeros(img.shape[:-1] + (4,), dtype=np.float32)
    out[..., :3] = (img.astype(np.float32) - mean) * denom
    return out


# ----------------------------------------------------------------------------- sample_params
def test_same_seed_same_tables_other_seed_or_rank_differs(aug):
    def tables(seed, rank):
        g = np.random.default_rng(np.random.SeedSequence(seed, spawn_key=(rank,)))
        return aug.sample_params(8, (37, 53), (24, 40), CONFIG, g)
    a, b = tables(3, 0), tables(3, 0)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert a[0].dtype == np.int32 and a[0].shape == (8, 16) and a[1].dtype == np.uint8 and a[1].shape == (8, 256)
    for other in (tables(4, 0), tables(3, 1)):
        assert not np.array_equal(a[0], other[0])
    # the DeviceAugment of one (seed, rank) holds that very generator
    d = aug.DeviceAugment(CONFIG, seed=3, rank=0)
    c = aug.sample_params(8, (37, 53), (24, 40), CONFIG, d.generator)
    assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1])


def test_draws_lie_inside_their_ranges_and_tables_follow(aug):
    g = np.random.default_rng(11)
    n = 400
    d = aug.draw_params(n, CONFIG, g)
    assert ((d['angle'] >= -10) & (d['angle'] <= 10)).all()
    assert np.isin(d['flip'], (0, 1, 2, 3)).all() and len(set(d['flip'].tolist())) == 4
    for k in ('dh', 'ds', 'dv'):
        assert d[k].min() == -10 and d[k].max() == 10                    # 400 draws of 21 values: both ends turn up
    assert ((np.abs(d['alpha'] - 1.0) <= 0.1) & (np.abs(d['beta']) <= 0.1)).all()
    for k in ('rotate', 'hsv', 'bc'):
        assert 0.35 < d[k].mean() < 0.65                                 # p = 0.5; 400 draws: 7.5 sigma is 0.19
    params, luts = aug.encode_params(d, (37, 53), (24, 40))
    ident = np.arange(256, dtype=np.uint8)
    for k in range(n):
        alpha, beta = float(d['alpha'][k]), float(d['beta'][k])
        want = np.clip(np.float32(np.arange(256)) * np.float32(alpha) + np.float32(beta * 255), 0, 255).astype(np.uint8) if d['bc'][k] else ident
        assert np.array_equal(luts[k], want)
        assert params[k, 6] == int(d['hsv'][k])
        assert tuple(params[k, 7:10]) == ((d['dh'][k], d['ds'][k], d['dv'][k]) if d['hsv'][k] else (0, 0, 0))
        assert not params[k, 10:].any()
        ar.check_row(params[k], 24, 40)
    # keyword limits
    d2 = aug.draw_params(200, CONFIG, np.random.default_rng(1), hue_shift_limit=2, sat_shift_limit=0, val_shift_limit=1, brightness_limit=0.0, contrast_limit=0.5)
    assert np.abs(d2['dh']).max() == 2 and not d2['ds'].any() and np.abs(d2['dv']).max() == 1
    assert not d2['beta'].any() and np.abs(d2['alpha'] - 1).max() > 0.1


def test_fixed_point_map_agrees_with_fp64_at_the_corners(aug):
    g = np.random.default_rng(2)
    for src_hw, out_hw in (((37, 53), (24, 40)), ((512, 512), (512, 512)), ((1024, 1024), (512, 512)), ((2, 2050), (2, 1025))):
        d = aug.draw_params(16, CONFIG, g)
        params, _ = aug.encode_params(d, src_hw, out_hw)
        for k in range(16):
            a = aug.affine_fp64(src_hw, out_hw, d['angle'][k] if d['rotate'][k] else 0.0, int(d['flip'][k]))
            m = params[k, :6].astype(np.int64)
            for i in (0, out_hw[0] - 1):
                for j in (0, out_hw[1] - 1):
                    want = a @ np.array([j, i, 1.0])
                    got = np.array([m[0] * j + m[1] * i + m[2], m[3] * j + m[4] * i + m[5]]) / 65536.0
                    # each of the six entries is off by at most 2^-17; the issue's bound 2^-16 (|i| + |j| + 1) covers it
                    assert (np.abs(got - want) <= 2.0 ** -16 * (i + j + 1)).all(), (src_hw, k, i, j, got, want)


# ----------------------------------------------------------------------------- augment_ref on exact cases
def test_identity_is_normalize(aug):
    img, mask = _source(9, 14)
    p, l = _rows(aug, (9, 14), (9, 14))
    assert tuple(p[0, :6]) == (65536, 0, 0, 0, 65536, 0)
    out, tgt = ar.augment_ref(img, mask, p, l, 9, 14)
    assert np.array_equal(out, _normalized(img))
    assert np.array_equal(tgt[..., :3], mask.astype(np.float32)) and not tgt[..., 3].any()


def test_flips_are_np_flip(aug):
    img, mask = _source(9, 14)
    for code, axes in ((aug.FLIP_H, (2,)), (aug.FLIP_V, (1,)), (aug.FLIP_BOTH, (1, 2))):
        p, l = _rows(aug, (9, 14), (9, 14), flip=code)
        out, tgt = ar.augment_ref(img, mask, p, l, 9, 14)
        assert np.array_equal(out, _normalized(np.flip(img, axes))), code
        assert np.array_equal(tgt[..., :3], np.flip(mask, axes).astype(np.float32)), code


def test_quarter_turns_are_np_rot90(aug):
    img, mask = _source(11, 11)
    for angle, k in ((90.0, 1), (-90.0, 3), (180.0, 2)):
        p, l = _rows(aug, (11, 11), (11, 11), angle=angle)
        assert all(abs(int(v)) in (0, 65536) for v in p[0, (0, 1, 3, 4)]) and not (p[0, (2, 5)] & 65535).any()
        out, tgt = ar.augment_ref(img, mask, p, l, 11, 11)
        assert np.array_equal(out, _normalized(np.rot90(img, k, axes=(1, 2)))), angle
        assert np.array_equal(tgt[..., :3], np.rot90(mask, k, axes=(1, 2)).astype(np.float32)), angle


def test_half_scale_is_the_mean_of_the_four_centre_taps(aug):
    img, mask = _source(8, 12)
    p, l = _rows(aug, (8, 12), (4, 6))
    assert tuple(p[0, :6]) == (131072, 0, 32768, 0, 131072, 32768)        # sx = 2 j + 1/2: x0 = 2 j, fx = 128
    out, tgt = ar.augment_ref(img, mask, p, l, 4, 6)
    v = img.astype(np.int64)
    box = (v[:, 0::2, 0::2] + v[:, 0::2, 1::2] + v[:, 1::2, 0::2] + v[:, 1::2, 1::2] + 2) >> 2     # (16384 sum + 32768) >> 16
    assert np.array_equal(out, _normalized(box.astype(np.uint8)))
    # nearest at the half-way point: (2 j + 1/2 + 1/2) floored = 2 j + 1
    assert np.array_equal(tgt[..., :3], mask[:, 1::2, 1::2].astype(np.float32))


def test_border_and_outside_taps(aug):
    img, mask = _source(4, 4)
    p = np.zeros((1, 16), dtype=np.int32)
    p[0, :6] = (65536, 0, -65536 - 32768, 0, 65536, 0)                     # sx = j - 3/2: x0 = -2, -1, 0, 1 with fx = 128
    l = np.tile(np.arange(256, dtype=np.uint8), (1, 1))
    out, tgt = ar.augment_ref(img, mask, p, l, 4, 4, border=(10, 20, 30))
    v = img[0].astype(np.int64)
    bd = np.array([10, 20, 30], dtype=np.int64)
    want = np.empty((4, 4, 3), dtype=np.int64)
    want[:, 0] = bd
    want[:, 1] = (bd + v[:, 0] + 1) >> 1
    want[:, 2] = (v[:, 0] + v[:, 1] + 1) >> 1
    want[:, 3] = (v[:, 1] + v[:, 2] + 1) >> 1
    assert np.array_equal(out[0], _normalized(want.astype(np.uint8)))
    want_m = np.zeros((4, 4, 3), dtype=np.float32)                         # nearest: (j - 3/2 + 1/2) = j - 1
    want_m[:, 1:] = mask[0, :, :3]
    assert np.array_equal(tgt[0, ..., :3], want_m)


def test_check_row_refuses_what_the_entry_refuses():
    row = np.zeros(16, dtype=np.int32)
    ar.check_row(row, 8, 8)
    for idx, val in ((6, 2), (6, 3), (7, 180), (8, -256), (9, 256)):
        bad = row.copy()
        bad[idx] = val
        with pytest.raises(ValueError):
            ar.check_row(bad, 8, 8)


def test_entry_refuses_bad_arguments_before_any_launch(pkg):
    """Host-side validation of ssg_augment_batch_u8_f32: a status and a message, nothing launched (so no GPU is needed; the
    pointers are host buffers that a kernel would never be given)."""
    import ctypes
    lib = pkg._lib
    img = np.zeros((1, 4, 4, 3), dtype=np.uint8)
    mask = np.zeros((1, 4, 4, 8), dtype=np.uint8)
    row = np.zeros((1, 16), dtype=np.int32)
    row[0, :6] = (65536, 0, 0, 0, 65536, 0)
    lut = np.arange(256, dtype=np.uint8).reshape(1, 256)
    out = np.zeros(4 * 4 * 8 + 4, dtype=np.float32)
    mean, denom = ar.norm_consts()

    def status(**kw):
        a = dict(img=img.ctypes.data, mask=mask.ctypes.data, N=1, H=4, W=4, C=3, params=row.ctypes.data, host=row.ctypes.data,
                 lut=lut.ctypes.data, out_h=4, out_w=4, border=(0, 0, 0), out_img=out.ctypes.data, out_tgt=out.ctypes.data)
        a.update(kw)
        rc = lib.load().ssg_augment_batch_u8_f32(a['img'], a['mask'], a['N'], a['H'], a['W'], a['C'], a['params'], a['host'], a['lut'],
                                                 a['out_h'], a['out_w'], *(list(a['border']) + [float(v) for v in mean] + [float(v) for v in denom]
                                                                          + [a['out_img'], a['out_tgt'], None]))
        return rc, lib.load().ssg_last_error()

    for kw in (dict(img=None), dict(mask=None), dict(params=None), dict(host=None), dict(lut=None), dict(out_img=None), dict(out_tgt=None),
               dict(N=0), dict(H=0), dict(W=-1), dict(out_h=0), dict(out_w=0), dict(C=0), dict(C=9), dict(border=(0, 256, 0)), dict(border=(-1, 0, 0))):
        rc, msg = status(**kw)
        assert rc != 0 and b'augment_batch' in msg, kw
    for idx, val in ((6, 2), (6, -1), (7, 180), (8, 256), (9, -256)):
        bad = row.copy()
        bad[0, idx] = val
        rc, msg = status(host=bad.ctypes.data)
        assert rc != 0 and b'augment_batch: sample 0' in msg, (idx, val)


# ----------------------------------------------------------------------------- HSV over all 2^24 colours
def _all_colours():
    for b in range(0, 256, 16):                                            # 16 slabs of 2^20 colours
        bb, g, r = np.meshgrid(np.arange(b, b + 16, dtype=np.int64), np.arange(256, dtype=np.int64), np.arange(256, dtype=np.int64), indexing='ij')
        yield bb.ravel(), g.ravel(), r.ravel()


def test_hsv_forward_equals_fp64_rounded_half_up():
    for b, g, r in _all_colours():
        h, s, v = ar.hsv_from_bgr(b, g, r)
        mx = np.maximum(np.maximum(b, g), r)
        d = mx - np.minimum(np.minimum(b, g), r)
        assert np.array_equal(v, mx)
        s64 = np.floor(255.0 * d / np.maximum(mx, 1) + 0.5).astype(np.int64)
        is_r = mx == r
        is_g = ~is_r & (mx == g)
        num = np.where(is_r, g - b, np.where(is_g, b - r, r - g))
        off = np.where(is_r, 0, np.where(is_g, 60, 120))
        h64 = np.floor(30.0 * num / np.maximum(d, 1) + 0.5).astype(np.int64) + off
        h64 = np.where(h64 < 0, h64 + 180, h64)
        h64 = np.where(d == 0, 0, h64)
        assert h.min() >= 0 and h.max() <= 179 and s.min() >= 0 and s.max() <= 255
        # a disagreement may only be an exact tie, which fp64 may not see as one: 2 * 255 d = (2 k + 1) V, 2 * 30 num = (2 k + 1) d
        bad = np.nonzero(s != s64)[0]
        assert ((510 * d[bad] - mx[bad]) % (2 * mx[bad]) == 0).all() and (np.abs(s[bad] - s64[bad]) <= 1).all(), 'S: %d colours differ off a tie' % len(bad)
        bad = np.nonzero(h != h64)[0]
        assert ((60 * num[bad] - d[bad]) % (2 * d[bad]) == 0).all() and (np.abs(h[bad] - h64[bad]) % 180 <= 1).all(), 'H: %d colours differ off a tie' % len(bad)


def test_hsv_round_trip_bound():
    worst = 0
    for b, g, r in _all_colours():
        b2, g2, r2 = ar.hsv_shift(b, g, r, 0, 0, 0)
        mx = np.maximum(np.maximum(b, g), r)
        assert np.array_equal(np.maximum(np.maximum(b2, g2), r2), mx)      # V is exact
        for x, y in ((b, b2), (g, g2), (r, r2)):
            assert y.min() >= 0 and y.max() <= 255
            worst = max(worst, int(np.abs(x - y).max()))
    print('HSV round trip, zero shifts, all 2^24 colours: max channel change', worst)
    assert worst <= 5                                                      # derived in the module docstring


def test_hsv_shift_extremes_stay_bytes():
    g = np.random.default_rng(0)
    px = g.integers(0, 256, (3, 20000))
    for dh, ds, dv in ((10, 10, 10), (-10, -10, -10), (179, 255, 255), (-179, -255, -255)):
        for ch in ar.hsv_shift(px[0], px[1], px[2], dh, ds, dv):
            assert ch.min() >= 0 and ch.max() <= 255
    b, g2, r = ar.hsv_shift(px[0], px[1], px[2], 0, 0, -255)               # V = 0 is black
    assert not b.any() and not g2.any() and not r.any()
    b, g2, r = ar.hsv_shift(px[0], px[1], px[2], 0, -255, 0)               # S = 0 is grey at V
    mx = px.max(axis=0)
    assert np.array_equal(b, mx) and np.array_equal(g2, mx) and np.array_equal(r, mx)
