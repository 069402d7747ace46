"""Device-side sliding-window inference (csrc/sliding_window.hip) against the host functions it restates: the gather kernel
against `get_patched_input`, the merge kernel against `patch_merge`, `segment_image` against `segmentation_inference_full`.
Everything is integer or single-rounding arithmetic, so every comparison is `np.array_equal` -- no tolerance."""
import numpy as np
import pytest
import torch

# (image H, W, patch, inference size): 70 x 75 puts the bottom / right anchored sweeps at origins 38, 22, 6 / 43, 27, 11 -- odd
# byte offsets into the 3-byte pixels, rows of 225 bytes -- at the factors 2 and 1; at 96 x 96 the four sweeps coincide
GEOMS = [(70, 75, 32, 16), (70, 75, 32, 32), (96, 96, 64, 32)]


def _cfg(p_size, size, classes=3):
    return dict(patch_size=p_size, input_w=size, input_h=size, patch_overlap=0.5, num_classes=classes)


def _image(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _raw(x):
    """The [N, H, W, ld] memory behind an NHWC tensor, pad lanes included."""
    n, c, h, w = x.shape
    ld = x.stride(3)
    return torch.empty(0, dtype=x.dtype, device=x.device).set_(x.untyped_storage(), x.storage_offset(), (n, h, w, ld)).cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize('h,w,p_size,size', GEOMS)
def test_gather_equals_get_patched_input_bit_for_bit(pkg, dev, h, w, p_size, size):
    A, ops = pkg.aerial_image_segmentation_api, pkg.ops
    img = _image(h, w, 21)
    _, want, _ = A.get_patched_input('image', _cfg(p_size, size), False, imread=lambda p: img)
    org = A.patch_origins(h, w, p_size, 0.5)
    x = ops.sw_gather_patches(torch.from_numpy(img).to(dev), org, p_size, size)
    assert tuple(x.shape) == want.shape == (len(org), 3, size, size) and ops.nhwc_ld(x) == 4
    raw = _raw(x)
    assert raw.shape == (len(org), size, size, 4)
    assert np.array_equal(raw[..., :3].transpose(0, 3, 1, 2), want)
    assert np.array_equal(x.cpu().numpy(), want)
    assert not raw[..., 3].view(np.int32).any()                             # pad lane: +0.0 exactly
    # consumed by the first convolution as it is: same values as the host path's upload + layout pass
    wt = torch.randn(4, 3, 3, 3, generator=torch.Generator().manual_seed(3)).to(dev)
    y = ops.conv2d(x, wt, padding=1)
    y_host_path = ops.conv2d(torch.from_numpy(want).to(dev), wt, padding=1)
    assert tuple(y.shape) == (len(org), 4, size, size) and torch.equal(y, y_host_path)


def _probs(kind, n, c, s, seed):
    rng = np.random.default_rng(seed)
    if kind == 'uniform':
        return rng.random((n, c, s, s), dtype=np.float32)
    # a field that lives on the thresholds: uint8 levels 120 .. 136 pushed just above / below the level by 1e-6 ...
    lv = rng.integers(120, 137, (n, c, s, s))
    p = (lv / 255.0 + rng.choice((-1e-6, 1e-6), lv.shape)).astype(np.float32)
    # ... the exact boundary values of the uint8 conversion ...
    for k, v in enumerate((0.0, 1.0, 127 / 255, 128 / 255)):
        p[:, :, 1 + k, 2] = np.float32(v)
        p[:, :, 0, 5 + k] = np.float32(v)
    # ... and neighbouring pairs whose 0.25 / 0.75 blends land on .25, .75 (127 | 128) and on .5 (126 | 132), on two equal rows
    for r, (a, b) in ((7, (127, 128)), (10, (126, 132)), (13, (128, 127))):
        p[:, :, r:r + 2, 3:9:2] = np.float32((a + 0.5) / 255)
        p[:, :, r:r + 2, 4:10:2] = np.float32((b + 0.5) / 255)
    return p


def _to_dev(ops, arr, dev):
    n, c, s, _ = arr.shape
    t = ops.new_nhwc(n, c, s, s, dev)
    t.copy_(torch.from_numpy(arr))
    return t


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['uniform', 'threshold'])
@pytest.mark.parametrize('classes', [1, 3])
@pytest.mark.parametrize('h,w,p_size,size', GEOMS)
def test_merge_equals_patch_merge_bit_for_bit(pkg, dev, h, w, p_size, size, classes, kind):
    A, ops = pkg.aerial_image_segmentation_api, pkg.ops
    org = A.patch_origins(h, w, p_size, 0.5)
    probs = _probs(kind, len(org), classes, size, 31)
    want = np.stack(A.patch_merge(np.zeros((h, w, 3), np.uint8), list(probs), p_size, dict(num_classes=classes), 0.5))
    got = ops.sw_merge_masks(_to_dev(ops, probs, dev), org, [1] * len(org), p_size, h, w)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (classes, h, w)
    got = got.cpu().numpy()
    for c in range(classes):
        assert set(np.unique(want[c])) == {0, 255}, 'class %d of the expected masks is constant: the case tests nothing' % c
    assert np.array_equal(got, want), 'differs at %d pixels' % int((got != want).sum())


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['uniform', 'threshold'])
@pytest.mark.parametrize('classes', [1, 3])
def test_merge_of_unique_origins_with_multiplicities_equals_host_on_the_duplicated_list(pkg, dev, classes, kind):
    A, ops = pkg.aerial_image_segmentation_api, pkg.ops
    h, w, p_size, size = GEOMS[2]
    org = A.patch_origins(h, w, p_size, 0.5)
    uniq, mult = A.unique_origins(org)
    assert len(org) == 16 and len(uniq) == 4 and mult == [4] * 4
    probs = _probs(kind, len(uniq), classes, size, 32)
    # unequal multiplicities too: drop one copy of one origin (the last sweep's last patch) from the host list
    for drop in (None, 15):
        full = [o for i, o in enumerate(org) if i != drop]
        wts = [full.count(o) for o in uniq]
        acc = np.zeros((classes, h, w)); div = np.zeros((h, w))
        for (h1, w1) in full:                                                # patch_merge's loop, for an arbitrary origin list
            m = probs[uniq.index((h1, w1))]
            u8 = np.stack([A.post_process_resized_mask(A.resize_u8((m[c] * 255).astype('uint8'), p_size, p_size)) for c in range(classes)])
            acc[:, h1:h1 + p_size, w1:w1 + p_size] += u8 / 255.0
            div[h1:h1 + p_size, w1:w1 + p_size] += 1.0
        div[div == 0] = 1.0
        want = np.stack([A.post_process_resized_mask((np.divide(acc[c], div) * 255).astype('uint8')) for c in range(classes)])
        if drop is None:
            assert np.array_equal(want, np.stack(A.patch_merge(np.zeros((h, w, 3), np.uint8), [probs[uniq.index(o)] for o in org],
                                                               p_size, dict(num_classes=classes), 0.5)))
        got = ops.sw_merge_masks(_to_dev(ops, probs, dev), uniq, wts, p_size, h, w).cpu().numpy()
        assert all(set(np.unique(want[c])) == {0, 255} for c in range(classes))
        assert np.array_equal(got, want), 'drop %s: differs at %d pixels' % (drop, int((got != want).sum()))


@pytest.fixture(scope='module')
def model(pkg, dev):
    torch.manual_seed(41)
    m = pkg.archs.UNet_R_SS_v2(3, 3, False).to(dev)
    m.train()
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        m(torch.randn(2, 3, 64, 64, generator=g).to(dev))                    # non-trivial running statistics
    return m.eval()


E2E = (192, 256, 128, 64)


@pytest.mark.gpu
def test_segment_image_without_dedupe_equals_the_host_pipeline(pkg, dev, model):
    """The same launch sequence on bit-identical inputs: 24 patches in batches of 6 on both paths."""
    A = pkg.aerial_image_segmentation_api
    h, w, p_size, size = E2E
    cfg, img = _cfg(p_size, size), _image(h, w, 22)
    full, patches, masks = A.get_patched_input('image', cfg, False, imread=lambda p: img)
    assert patches.shape == (24, 3, size, size)
    want = A.segmentation_inference_full(model, full, patches, masks, cfg, False, batch_size=6)[0]
    got = A.segment_image(model, img, cfg, batch_size=6, dedupe=False)
    assert len(got) == 3 and all(g.dtype == np.uint8 and g.shape == (h, w) for g in got)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))


@pytest.mark.gpu
@pytest.mark.parametrize('batch_size', [6, 4])
def test_segment_image_dedupe_merges_each_unique_origin_with_its_multiplicity(pkg, dev, model, batch_size):
    """6 unique origins of 24 (batch 4: a partial last batch): the masks are the host `patch_merge` of the returned
    probabilities, each standing for its 4 duplicates -- however the forward rounds."""
    A = pkg.aerial_image_segmentation_api
    h, w, p_size, size = E2E
    cfg, img = _cfg(p_size, size), _image(h, w, 22)
    got, probs, org, wts = A.segment_image(model, img, cfg, batch_size=batch_size, dedupe=True, return_probs=True)
    full_org = A.patch_origins(h, w, p_size, 0.5)
    assert (org, wts) == A.unique_origins(full_org) and len(org) == 6 and wts == [4] * 6
    assert probs.shape == (6, 3, size, size) and probs.dtype == np.float32 and 0.0 <= probs.min() and probs.max() <= 1.0
    want = A.patch_merge(img, [probs[org.index(o)] for o in full_org], p_size, cfg, 0.5)
    assert len(got) == 3 and all(np.array_equal(a, b) for a, b in zip(got, want))
    # and the probabilities are the model's: the host path on the same six patches in the same batches
    _, patches, _ = A.get_patched_input('image', cfg, False, imread=lambda p: img)
    first = [full_org.index(o) for o in org]
    assert np.array_equal(probs, A.infer_patches(model, patches[first], batch_size=batch_size).numpy())


@pytest.mark.gpu
def test_wrappers_raise_before_any_launch(pkg, dev):
    ops = pkg.ops
    img = torch.from_numpy(_image(96, 96, 23))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.sw_gather_patches(img, [(0, 0)], 64, 32)                         # image on the host
    with pytest.raises(NotImplementedError):
        ops.sw_gather_patches(img.to(dev), [(0, 0)], 64, 16)                 # factor 4
    with pytest.raises(ValueError, match='outside'):
        ops.sw_gather_patches(img.to(dev), [(0, 0), (33, 0)], 64, 32)        # 33 + 64 > 96
    with pytest.raises(ValueError, match='outside'):
        ops.sw_gather_patches(img.to(dev), [(-1, 0)], 64, 32)
    probs = ops.new_nhwc(1, 3, 16, 16, dev, zero=True)
    with pytest.raises(NotImplementedError):
        ops.sw_merge_masks(probs, [(0, 0)], [1], 64, 96, 96)                 # factor 4
    with pytest.raises(ValueError, match='outside'):
        ops.sw_merge_masks(probs, [(0, 80)], [1], 32, 96, 96)
    with pytest.raises(ValueError):
        ops.sw_merge_masks(probs, [(0, 0), (0, 16)], [1, 1], 32, 96, 96)     # two origins for one patch
