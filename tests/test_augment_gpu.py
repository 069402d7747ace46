"""GPU: ops.augment_batch / ssg_augment_batch_u8_f32 and augment.DeviceAugment against tests/augment_ref.py, byte for byte
(torch.equal on the whole NHWC memory, pad lanes included: no tolerance, no excused share), and the opt-in wiring of the two
trainers.  Shapes are the smallest that take every path: a 37 x 53 source (odd, not square, rows of 159 bytes) to 24 x 40 (960
pixels: four workgroups per sample, the last one partly idle), three samples with three different rows in one launch, C = 1, 3
and 5 (target ld 4 and 8)."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn

import augment_ref as ar

pytestmark = pytest.mark.gpu

SRC, OUT = (37, 53), (24, 40)
CONFIG = dict(rotate_min=-10, rotate_max=10, input_h=OUT[0], input_w=OUT[1])


def _memory(t):
    """The [N, H, W, ld] memory of a new_nhwc tensor, pad lanes included."""
    n, c, h, w = t.shape
    ld = (c + 3) // 4 * 4
    assert t.stride() == (h * w * ld, 1, w * ld, ld)
    return torch.as_strided(t, (n, h, w, ld), (h * w * ld, w * ld, ld, 1)).cpu()


def _tiles(n, hw, c, seed=3):
    g = np.random.default_rng(seed)
    return g.integers(0, 256, (n, hw[0], hw[1], 3), dtype=np.uint8), g.integers(0, 2, (n, hw[0], hw[1], c), dtype=np.uint8) * 255


def _row(aug, src_hw, out_hw, angle=0.0, zoom=1.0, flip=0, hsv=None):
    """A parameter row: the trainer's map for (angle, flip), every output pixel moved towards (zoom < 1) or away from (zoom > 1)
    the output centre first -- zoom 2 sends the corners well outside the source."""
    a = np.vstack([aug.affine_fp64(src_hw, out_hw, angle, flip), [0, 0, 1]])
    cy, cx = (out_hw[0] - 1) / 2.0, (out_hw[1] - 1) / 2.0
    z = np.array([[zoom, 0, cx - zoom * cx], [0, zoom, cy - zoom * cy], [0, 0, 1]])
    row = np.zeros(16, dtype=np.int32)
    row[:6] = aug.fixed_map((a @ z)[:2])
    if hsv is not None:
        row[6:10] = (1,) + tuple(hsv)
    return row


def _check(pkg, dev, img, mask, params, luts, out_hw, border=(0, 0, 0)):
    want_i, want_t = ar.augment_ref(img, mask, params, luts, out_hw[0], out_hw[1], border)
    got_i, got_t = pkg.ops.augment_batch(torch.from_numpy(img).to(dev), torch.from_numpy(mask).to(dev), params, luts, out_hw[0], out_hw[1], border=border)
    assert got_i.shape == (img.shape[0], 3, out_hw[0], out_hw[1]) and got_t.shape == (img.shape[0], mask.shape[3], out_hw[0], out_hw[1])
    assert pkg.ops.nhwc_ld(got_i) == 4 and pkg.ops.nhwc_ld(got_t) == want_t.shape[-1]
    assert torch.equal(_memory(got_i), torch.from_numpy(want_i))
    assert torch.equal(_memory(got_t), torch.from_numpy(want_t))
    return want_i, want_t


IDENT = np.arange(256, dtype=np.uint8)
SETS = {
    # (angle, zoom, flip, hsv shifts or None, (alpha, beta) or None) x 3 samples, border
    'angles_0_p10_m10': ([(0.0, 1.0, 0, None, None), (10.0, 0.5, 1, (10, 10, 10), (1.1, 0.1)), (-10.0, 1.5, 2, (-10, -10, -10), (0.9, -0.1))], (0, 0, 0)),
    'angles_45_180_zoom2': ([(45.0, 2.0, 0, (-10, 10, -10), (1.1, -0.1)), (180.0, 1.0, 3, None, (0.9, 0.1)), (10.0, 2.0, 0, (10, -10, 10), None)], (10, 200, 77)),
}


@pytest.mark.parametrize('c', [1, 3, 5])
@pytest.mark.parametrize('name', sorted(SETS))
def test_three_rows_in_one_launch(pkg, dev, name, c):
    aug = pkg.augment
    rows, border = SETS[name]
    img, mask = _tiles(3, SRC, c)
    params = np.stack([_row(aug, SRC, OUT, a, z, f, hsv) for a, z, f, hsv, _ in rows])
    luts = np.stack([IDENT if bc is None else aug.bc_lut(*bc) for _, _, _, _, bc in rows])
    want_i, want_t = _check(pkg, dev, img, mask, params, luts, OUT, border)
    # the cases are not degenerate: three different samples, and border pixels where the set promises them
    assert not np.array_equal(want_i[0], want_i[1]) and not np.array_equal(want_i[1], want_i[2])
    assert want_t[..., :c].any() and not want_t[..., c:].any()
    if name == 'angles_45_180_zoom2':                                           # zoom 2: the output corners lie outside the source
        assert not want_t[0, 0, 0].any() and not want_t[2, 0, 0].any() and not want_t[0, -1, -1].any()


def test_plain_scales(pkg, dev):
    """The trainer's own scale maps, no rotation: source / output = 1/2, 1, 3/2 and 2 per axis."""
    aug = pkg.augment
    for src_hw, out_hw in (((12, 20), (24, 40)), ((24, 40), (24, 40)), ((36, 60), (24, 40)), ((48, 80), (24, 40)), (SRC, OUT)):
        img, mask = _tiles(2, src_hw, 3, seed=8)
        params, luts = aug.plain_params(2, src_hw, out_hw)
        _check(pkg, dev, img, mask, params, luts, out_hw)


def test_edge_straddle_and_border(pkg, dev):
    """sx = j - 3/2 on a 5 x 7 source, 9 columns out: base taps x0 = -2 .. 6, so (-1, 0) and (W - 1, W) straddle the two edges
    with weight 1/2 each side; sy = i - 1/2 does the same to the rows."""
    img, mask = _tiles(1, (5, 7), 3, seed=9)
    params = np.zeros((1, 16), dtype=np.int32)
    params[0, :6] = (65536, 0, -98304, 0, 65536, -32768)
    luts = IDENT[None].copy()
    for border in ((0, 0, 0), (255, 1, 128)):
        want_i, _ = _check(pkg, dev, img, mask, params, luts, (6, 9), border)
    v = img[0].astype(np.int64)
    mean, denom = ar.norm_consts()
    # written out for one pixel: output (1, 8) blends source (0, 6), (1, 6) and two border taps, a quarter each
    px = (v[0, 6] + v[1, 6] + 2 * np.array([255, 1, 128]) + 2) >> 2
    assert np.array_equal(want_i[0, 1, 8, :3], (px.astype(np.float32) - mean) * denom)


def test_colour_stage_extremes(pkg, dev):
    """HSV on and off with the extreme shifts, tables that saturate at both ends, on every grey and a colour ramp."""
    aug = pkg.augment
    g = np.random.default_rng(4)
    img = g.integers(0, 256, (6, 16, 64, 3), dtype=np.uint8)
    img[:, 0, :, :] = (np.arange(64, dtype=np.uint8) * 4)[None, :, None]         # greys: d = 0
    img[:, 1, :, 0] = 255                                                       # saturated primaries and black
    img[:, 1, :, 1:] = 0
    img[:, 2] = 0
    img[:, 3] = 255
    mask = g.integers(0, 256, (6, 16, 64, 2), dtype=np.uint8)
    params, luts = aug.plain_params(6, (16, 64), (16, 64))
    for k, hsv in enumerate(((10, 10, 10), (-10, -10, -10), (10, -10, 10), None, (179, 255, 255), (-179, -255, -255))):
        if hsv is not None:
            params[k, 6:10] = (1,) + hsv
    luts[0] = aug.bc_lut(1.1, 0.1)
    luts[1] = aug.bc_lut(0.9, -0.1)
    luts[2] = 255 - IDENT                                                       # any table: the kernel only indexes it
    luts[3] = aug.bc_lut(1.1, -0.1)
    assert luts[0].max() == 255 and (luts[0] == 255).sum() > 20 and (luts[1] == 0).sum() > 20
    _check(pkg, dev, img, mask, params, luts, (16, 64))


def test_int64_coordinates(pkg, dev):
    """A 2 x 2050 source.  Sample 0 steps 32 source pixels per output column from 32768 pixels left of the source: m0 j passes
    2^31 inside the stretch of columns that read the source (1018 .. 1081), so a 32-bit product would put those elsewhere.  Sample 1 is
    the left-right flip at full width."""
    aug = pkg.augment
    img, mask = _tiles(2, (2, 2050), 1, seed=6)
    params = np.zeros((2, 16), dtype=np.int32)
    params[0, :6] = ((1 << 21) + 12345, 0, -(1 << 31) + 777, 0, 65536, 0)
    params[1, :6] = aug.fixed_map(aug.affine_fp64((2, 2050), (2, 2050), 0.0, aug.FLIP_H))
    luts = np.stack([IDENT, IDENT])
    mask[:] = 255
    want_i, want_t = _check(pkg, dev, img, mask, params, luts, (2, 2050), border=(7, 8, 9))
    inside = np.nonzero(want_t[0, 0, :, 0] > 0)[0]
    assert 60 <= len(inside) <= 66 and int(params[0, 0]) * int(inside.max()) >= 1 << 31 > int(params[0, 0]) * int(inside.min())


def test_bad_inputs_raise_before_any_launch(pkg, dev):
    aug = pkg.augment
    img, mask = _tiles(2, SRC, 3)
    params, luts = aug.plain_params(2, SRC, OUT)
    gi, gm = torch.from_numpy(img).to(dev), torch.from_numpy(mask).to(dev)
    out = (pkg.ops.new_nhwc(2, 3, OUT[0], OUT[1], dev), pkg.ops.new_nhwc(2, 3, OUT[0], OUT[1], dev))
    for t in out:
        _memory_view = torch.as_strided(t, (2, OUT[0], OUT[1], 4), (OUT[0] * OUT[1] * 4, OUT[1] * 4, 4, 1))
        _memory_view.fill_(-7.0)
    wide = torch.from_numpy(np.ascontiguousarray(np.concatenate([img, img], axis=2))).to(dev)
    cases = [
        (TypeError, dict(img=wide[:, :, ::2])),                                 # right shape, not contiguous
        (TypeError, dict(img=gi.permute(0, 2, 1, 3))),                          # not contiguous, wrong shape
        (TypeError, dict(img=gi.to(torch.int8))), (TypeError, dict(img=gi.float())),
        (TypeError, dict(mask=gm.float())), (TypeError, dict(mask=gm[:, :, :, ::2])), (TypeError, dict(mask=gm[:1])),
        (TypeError, dict(params=params.astype(np.int64))), (TypeError, dict(params=params[:1])), (TypeError, dict(luts=luts[:, :128])),
        (ValueError, dict(border=(0, 0, 256))), (ValueError, dict(out_h=0)),
    ]
    bad_flags = params.copy()
    bad_flags[1, 6] = 4
    cases.append((pkg._lib.HipLibraryError, dict(params=bad_flags)))            # refused by the entry point's host-side check
    for exc, kw in cases:
        a = dict(img=gi, mask=gm, params=params, luts=luts, out_h=OUT[0], out_w=OUT[1], border=(0, 0, 0))
        a.update(kw)
        with pytest.raises(exc):
            pkg.ops.augment_batch(a['img'], a['mask'], a['params'], a['luts'], a['out_h'], a['out_w'], border=a['border'], out=out)
    with pytest.raises(RuntimeError):
        pkg.ops.augment_batch(torch.from_numpy(img), torch.from_numpy(mask), params, luts, OUT[0], OUT[1])     # CPU tensors
    torch.cuda.synchronize()
    for t in out:
        assert bool((_memory(t) == -7.0).all())
    # and the same buffers are written by a good call
    got = pkg.ops.augment_batch(gi, gm, params, luts, OUT[0], OUT[1], out=out)
    assert got[0] is out[0] and got[1] is out[1]
    want_i, want_t = ar.augment_ref(img, mask, params, luts, OUT[0], OUT[1])
    assert torch.equal(_memory(out[0]), torch.from_numpy(want_i)) and torch.equal(_memory(out[1]), torch.from_numpy(want_t))


# ----------------------------------------------------------------------------- DeviceAugment
def test_device_augment_seed_val_transform_and_float_form(pkg, dev):
    aug = pkg.augment
    img, mask = _tiles(4, SRC, 3, seed=12)
    mask = mask // 255
    gi, gm = torch.from_numpy(img).to(dev), torch.from_numpy(mask).to(dev)
    a, b = aug.DeviceAugment(CONFIG, seed=5), aug.DeviceAugment(CONFIG, seed=5)
    ia, ta = a(gi, gm)
    ib, tb = b(gi, gm)
    assert torch.equal(_memory(ia), _memory(ib)) and torch.equal(_memory(ta), _memory(tb))
    # ... and is the definition at the parameters that seed draws
    params, luts = aug.sample_params(4, SRC, OUT, CONFIG, aug.DeviceAugment(CONFIG, seed=5).generator)
    want_i, want_t = ar.augment_ref(img, mask, params, luts, OUT[0], OUT[1])
    assert torch.equal(_memory(ia), torch.from_numpy(want_i)) and torch.equal(_memory(ta), torch.from_numpy(want_t))
    ic, _ = aug.DeviceAugment(CONFIG, seed=6)(gi, gm)
    id_, _ = aug.DeviceAugment(CONFIG, seed=5, rank=1)(gi, gm)
    assert not torch.equal(_memory(ia), _memory(ic)) and not torch.equal(_memory(ia), _memory(id_))
    # train=False: the plain scale map, no colour stage
    val = aug.DeviceAugment(CONFIG, train=False)
    assert a.validation() is a.validation() and a.validation().train is False and val.validation() is val
    iv, tv = val(gi, gm)
    p = np.zeros((4, 16), dtype=np.int32)
    p[:, :6] = aug.fixed_map(aug.affine_fp64(SRC, OUT))
    want_i, want_t = ar.augment_ref(img, mask, p, np.tile(IDENT, (4, 1)), OUT[0], OUT[1])
    assert torch.equal(_memory(iv), torch.from_numpy(want_i)) and torch.equal(_memory(tv), torch.from_numpy(want_t))
    iv2, tv2 = a.validation()(gi, gm)
    assert torch.equal(_memory(iv2), _memory(iv)) and torch.equal(_memory(tv2), _memory(tv))
    # what Dataset(transform=None) collates: float32 NCHW holding the same integers
    fi = torch.from_numpy(img.astype(np.float32).transpose(0, 3, 1, 2).copy()).to(dev)
    fm = torch.from_numpy(mask.astype(np.float32).transpose(0, 3, 1, 2).copy()).to(dev)
    i_f, t_f = aug.DeviceAugment(CONFIG, seed=5)(fi, fm)
    assert torch.equal(_memory(i_f), _memory(ia)) and torch.equal(_memory(t_f), _memory(ta))
    for bad_i, bad_m in ((fi + 0.5, fm), (fi - 1.0, fm), (fi + 1.0, fm), (fi, fm * 2.0), (fi, fm * 0.5)):
        with pytest.raises(ValueError):
            aug.DeviceAugment(CONFIG, seed=5)(bad_i, bad_m)


# ----------------------------------------------------------------------------- the trainers
WIRE = dict(rotate_min=-10, rotate_max=10, input_h=64, input_w=64, num_classes=3, clip=0.7, deep_supervision=False)


def _loader():
    g = np.random.default_rng(21)
    return [(None, torch.from_numpy(g.integers(0, 256, (2, 64, 64, 3), dtype=np.uint8)),
             torch.from_numpy(g.integers(0, 2, (2, 64, 64, 3), dtype=np.uint8)), None, None) for _ in range(2)]


def test_gan_trainer_applies_device_augment(pkg, dev):
    """train_seg_gan.train over two 2 x 64^2 uint8 batches with config['device_augment'] == gan_step fed by hand with the output
    of a DeviceAugment of the same seed, on copies of the same models: the three returned numbers, with ==."""
    T = pkg.train_seg_gan
    torch.manual_seed(41)
    G = pkg.models_seg_gan.Generator(dict(arch='UNet_R_SS_v2', num_classes=3, input_channels=3, deep_supervision=False)).to(dev)
    D = pkg.models_seg_gan.Discriminator(3, kernel_size=3, n_channels=64, n_blocks=8, fc_size=1024).to(dev)
    G2, D2 = copy.deepcopy(G), copy.deepcopy(D)
    crit, adv, con = pkg.losses.BCEDiceLoss(), nn.BCEWithLogitsLoss(), nn.MSELoss()
    loader = _loader()

    og, od = torch.optim.Adam(G.parameters(), lr=2e-5), torch.optim.Adam(D.parameters(), lr=2e-5)
    config = dict(WIRE, device_augment=pkg.augment.DeviceAugment(WIRE, seed=9))
    got = T.train(0, config, loader, G, D, crit, adv, con, og, od)

    og, od = torch.optim.Adam(G2.parameters(), lr=2e-5), torch.optim.Adam(D2.parameters(), lr=2e-5)
    hand = pkg.augment.DeviceAugment(WIRE, seed=9)
    G2.train(); D2.train()
    meters = [pkg.utils.AverageMeter() for _ in range(3)]
    for _, img, mask, _, _ in loader:
        inp, tgt = hand(img.to(dev), mask.to(dev))
        loss, iou, dice, _, _, _ = T.gan_step(inp, tgt, G2, D2, crit, adv, con, og, od, 3)
        for m, v in zip(meters, (loss, iou, dice)):
            m.update(v, inp.size(0))
    want = [float(m.avg.item()) for m in meters]
    assert [got['loss'], got['iou'], got['dice']] == want
    assert all(np.isfinite(v) for v in want)
    # validate() takes the train=False twin: equal to a validate() over tensors that twin made
    rv = T.validate(config, loader, G, crit)
    val = pkg.augment.DeviceAugment(WIRE, train=False)
    pre = [(None,) + val(img.to(dev), mask.to(dev)) + (None, None) for _, img, mask, _, _ in loader]
    assert rv == T.validate(dict(WIRE), pre, G, crit)


def test_stage1_trainer_applies_device_augment(pkg, dev):
    """The same for train.train: with config['device_augment'] on uint8 batches == without the key on the tensors a DeviceAugment
    of the same seed made from them."""
    torch.manual_seed(41)
    model = pkg.archs.UNet_R_SS_v2(3, 3, False).to(dev)
    model2 = copy.deepcopy(model)
    loader = _loader()
    crit = pkg.losses.BCEDiceLoss()
    config = dict(WIRE, device_augment=pkg.augment.DeviceAugment(WIRE, seed=9))
    got = pkg.train.train(0, config, loader, model, crit, torch.optim.Adam(model.parameters(), lr=1e-4, weight_decay=1e-7), None)
    hand = pkg.augment.DeviceAugment(WIRE, seed=9)
    pre = [(None,) + hand(img.to(dev), mask.to(dev)) + (None, None) for _, img, mask, _, _ in loader]
    want = pkg.train.train(0, dict(WIRE), pre, model2, crit, torch.optim.Adam(model2.parameters(), lr=1e-4, weight_decay=1e-7), None)
    assert got == want and all(np.isfinite(v) for v in got.values())
    rv = pkg.train.validate(config, loader, model, crit)
    val = pkg.augment.DeviceAugment(WIRE, train=False)
    pre = [(None,) + val(img.to(dev), mask.to(dev)) + (None, None) for _, img, mask, _, _ in loader]
    assert rv == pkg.train.validate(dict(WIRE), pre, model, crit)
