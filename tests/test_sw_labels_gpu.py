"""The ground-truth branch of sliding-window inference on the device (csrc/sliding_window.hip) against the host functions it
restates: `ops.sw_gather_labels` against `mask_convert`, gather + merge against the host `patch_merge` of the host labels,
`segment_image(..., label_bgr=)` against `segmentation_inference_full(..., gt_mask_flag=True)`, `ops.sw_mask_counts` and the
evaluation functions against numpy.  Every value is an integer: every comparison is `np.array_equal`.  The label images are
those of tests/test_sw_labels_host.py, whose rehearsal shows on the host that they can tell a wrong kernel from a right one."""
import numpy as np
import pytest
import torch

from test_sliding_window_gpu import E2E, _image, _raw, model  # noqa: F401  (model: the seeded UNet_R_SS_v2 fixture)
from test_sw_labels_host import GEOMS, SEED, cfg, host_gt_masks, host_labels, label_image


@pytest.mark.gpu
@pytest.mark.parametrize('classes', [1, 3])
@pytest.mark.parametrize('block', [1, 3])
@pytest.mark.parametrize('h,w,p_size,size', GEOMS)
def test_label_gather_equals_mask_convert_and_merges_like_the_host(pkg, dev, h, w, p_size, size, block, classes):
    A, ops = pkg.aerial_image_segmentation_api, pkg.ops
    lab = label_image(h, w, block, SEED + block)
    want = host_labels(A, lab, p_size, size, classes)
    org = A.patch_origins(h, w, p_size, 0.5)
    x = ops.sw_gather_labels(torch.from_numpy(lab).to(dev), org, p_size, size, classes)
    assert tuple(x.shape) == want.shape == (len(org), classes, size, size) and x.dtype == torch.float32 and ops.nhwc_ld(x) == 4
    raw = _raw(x)
    assert raw.shape == (len(org), size, size, 4)
    for c in range(classes):
        assert set(np.unique(want[:, c])) == {0.0, 1.0}, 'class %d of the expected patches is constant' % c
    assert np.array_equal(raw[..., :classes].transpose(0, 3, 1, 2), want.astype(np.float32))
    assert np.array_equal(x.cpu().numpy().astype(np.float64), want)
    assert set(np.unique(raw.view(np.int32))) == {0, 0x3f800000}             # +0.0 or 1.0 bit-wise, pad lanes included ...
    assert not raw[..., classes:].view(np.int32).any()                       # ... and the pad lanes +0.0
    # gather then merge, unit weights: the host patch_merge of the host labels
    got = ops.sw_merge_masks(x, org, [1] * len(org), p_size, h, w).cpu().numpy()
    want_masks = host_gt_masks(A, lab, p_size, size, classes)
    assert all(set(np.unique(want_masks[c])) == {0, 255} for c in range(classes))
    assert np.array_equal(got, want_masks), 'differs at %d pixels' % int((got != want_masks).sum())


def _e2e_pair(seed=22, block=3):
    h, w, p_size, size = E2E
    return _image(h, w, seed), label_image(h, w, block, SEED + 10 + seed)


@pytest.mark.gpu
def test_segment_image_with_label_without_dedupe_equals_the_host_pipeline(pkg, dev, model):
    """Both lists of the host pipeline with gt_mask_flag=True: 24 patches in batches of 6 on both paths."""
    A = pkg.aerial_image_segmentation_api
    h, w, p_size, size = E2E
    cfg_, (img, lab) = cfg(p_size, size), _e2e_pair()
    want, want_gt = A.segmentation_inference_full(
        model, *A.get_patched_input('image', cfg_, True, imread=lambda p: lab if 'labels' in p else img), cfg_, True, batch_size=6)
    res = A.segment_image(model, img, cfg_, batch_size=6, dedupe=False, label_bgr=lab)
    assert isinstance(res, tuple) and len(res) == 2
    got, got_gt = res
    for masks in (got, got_gt):
        assert len(masks) == 3 and all(g.dtype == np.uint8 and g.shape == (h, w) for g in masks)
    assert all(set(np.unique(m)) == {0, 255} for m in want_gt)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    assert all(np.array_equal(a, b) for a, b in zip(got_gt, want_gt))
    assert not any(np.array_equal(a, b) for a, b in zip(want, want_gt))      # two different mask sets
    # without the new argument: the masks alone, as before
    plain = A.segment_image(model, img, cfg_, batch_size=6, dedupe=False)
    assert isinstance(plain, list) and all(np.array_equal(a, b) for a, b in zip(plain, want))


@pytest.mark.gpu
def test_ground_truth_masks_depend_on_neither_dedupe_nor_precision(pkg, dev, model):
    A = pkg.aerial_image_segmentation_api
    h, w, p_size, size = E2E
    cfg_, (img, lab) = cfg(p_size, size), _e2e_pair()
    _, base = A.segment_image(model, img, cfg_, batch_size=6, dedupe=False, label_bgr=lab)
    assert np.array_equal(np.stack(base), host_gt_masks(A, lab, p_size, size, 3))
    res = A.segment_image(model, img, cfg_, batch_size=6, dedupe=True, label_bgr=lab, return_probs=True)
    assert len(res) == 5
    masks, gt, probs, org, wts = res
    assert len(org) == 6 and wts == [4] * 6 and probs.shape == (6, 3, size, size)
    assert all(np.array_equal(a, b) for a, b in zip(gt, base))
    assert all(np.array_equal(a, b) for a, b in zip(masks, A.segment_image(model, img, cfg_, batch_size=6, dedupe=True)))
    for dedupe in (True, False):
        _, gt16 = A.segment_image(model, img, cfg_, batch_size=6, dedupe=dedupe, precision='bf16x1', label_bgr=lab)
        assert all(np.array_equal(a, b) for a, b in zip(gt16, base))


def _planes(classes, hw, off, seed, dev):
    """uint8 [classes, hw] on the device whose first byte sits `off` bytes behind a 16-byte boundary, with its host copy."""
    host = np.random.default_rng(seed).integers(0, 256, (classes, hw), dtype=np.uint8)
    host[:, 0], host[:, hw // 2], host[:, -1] = 127, 128, 127                # both sides of the threshold, in every plane
    buf = torch.zeros(classes * hw + 32, dtype=torch.uint8, device=dev)
    start = (-buf.data_ptr()) % 16 + off
    t = buf[start:start + classes * hw].view(classes, hw)
    t.copy_(torch.from_numpy(host))
    assert t.data_ptr() % 16 == off % 16 and t.is_contiguous()
    return t, host


# (classes, H * W, byte offsets of the two sets): equal offsets take 16 bytes per thread between a byte head and tail, unequal
# ones go byte by byte; 5250 = 70 * 75 puts planes 1 and 2 off the boundary by themselves; 131229 pixels spread over 3 blocks of 64 KiB
@pytest.mark.gpu
@pytest.mark.parametrize('classes,hw,offs', [(3, 5250, (1, 1)), (3, 5250, (3, 5)), (3, 5250, (0, 0)), (1, 37, (7, 7)), (1, 37, (0, 9)),
                                              (3, 65536 * 2 + 157, (13, 13)), (2, 65536 * 2 + 157, (0, 4))])
def test_mask_counts_equal_numpy(pkg, dev, classes, hw, offs):
    ops = pkg.ops
    pred, hp = _planes(classes, hw, offs[0], 51, dev)
    gt, hg = _planes(classes, hw, offs[1], 52, dev)
    for c in range(classes):
        assert len(np.unique(hp[c] > 127)) == 2 and len(np.unique(hg[c] > 127)) == 2
    assert (hp == 127).any() and (hp == 128).any() and (hg == 127).any() and (hg == 128).any()
    want = np.stack([((hp > 127) & (hg > 127)).sum(1), (hp > 127).sum(1), (hg > 127).sum(1)], 1).astype(np.int64)
    assert not np.array_equal(want, np.stack([((hp >= 127) & (hg >= 127)).sum(1), (hp >= 127).sum(1), (hg >= 127).sum(1)], 1))
    got = ops.sw_mask_counts(pred, gt)
    assert got.dtype == torch.int64 and tuple(got.shape) == (classes, 3) and got.is_cuda
    assert np.array_equal(got.cpu().numpy(), want)
    again = ops.sw_mask_counts(pred, gt, out=got)                            # accumulates
    assert again is got and np.array_equal(got.cpu().numpy(), 2 * want)
    if hw == 5250:                                                           # [C, H, W] as the merge leaves it
        assert np.array_equal(ops.sw_mask_counts(pred.view(classes, 70, 75), gt.view(classes, 70, 75)).cpu().numpy(), want)


def _host_counts(masks, gt):
    return np.array([[int(((m > 127) & (g > 127)).sum()), int((m > 127).sum()), int((g > 127).sum())] for m, g in zip(masks, gt)], dtype=np.int64)


@pytest.mark.gpu
def test_evaluate_image_and_images_equal_counts_taken_on_the_host(pkg, dev, model, monkeypatch):
    A = pkg.aerial_image_segmentation_api
    h, w, p_size, size = E2E
    cfg_ = cfg(p_size, size)
    pairs = [_e2e_pair(22, 3), _e2e_pair(23, 5)]
    assert not np.array_equal(pairs[0][0], pairs[1][0]) and not np.array_equal(pairs[0][1], pairs[1][1])
    want = [_host_counts(*A.segment_image(model, img, cfg_, batch_size=6, label_bgr=lab)) for img, lab in pairs]
    print('host counts (I, P, G) per class:', [wc.tolist() for wc in want])
    assert all((wc[:, 2] > 0).all() for wc in want) and not np.array_equal(want[0], want[1])
    got = A.evaluate_image(model, pairs[0][0], pairs[0][1], cfg_, batch_size=6)
    assert got.is_cuda and got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want[0])
    acc = A.evaluate_image(model, pairs[1][0], pairs[1][1], cfg_, batch_size=6, counts=got)
    assert acc is got and np.array_equal(got.cpu().numpy(), want[0] + want[1])
    # the second pair as paths
    files = {'image/b.png': pairs[1][0], 'labels/b.png': pairs[1][1]}
    monkeypatch.setattr(A, 'imread_bgr', lambda p: files[p])
    res = A.evaluate_images(model, [pairs[0], ('image/b.png', 'labels/b.png')], cfg_, batch_size=6)
    total = want[0] + want[1]
    assert isinstance(res['counts'], np.ndarray) and res['counts'].dtype == np.int64 and np.array_equal(res['counts'], total)
    for c, (i, p, g) in enumerate(total.tolist()):
        assert isinstance(res['iou'][c], float) and res['iou'][c] == (i + 1e-5) / (p + g - i + 1e-5)
        assert isinstance(res['dice'][c], float) and res['dice'][c] == (2 * i + 1e-5) / (p + g + 1e-5)
    assert len(res['iou']) == len(res['dice']) == 3


@pytest.mark.gpu
def test_label_wrappers_raise_before_any_launch(pkg, dev, model):
    A, ops = pkg.aerial_image_segmentation_api, pkg.ops
    lab = torch.from_numpy(label_image(96, 96, 1, SEED))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.sw_gather_labels(lab, [(0, 0)], 64, 32)                          # label on the host
    with pytest.raises(NotImplementedError):
        ops.sw_gather_labels(lab.to(dev), [(0, 0)], 64, 16)                  # factor 4
    with pytest.raises(ValueError, match='classes'):
        ops.sw_gather_labels(lab.to(dev), [(0, 0)], 64, 32, classes=4)
    with pytest.raises(ValueError, match='classes'):
        ops.sw_gather_labels(lab.to(dev), [(0, 0)], 64, 32, classes=0)
    with pytest.raises(ValueError, match='outside'):
        ops.sw_gather_labels(lab.to(dev), [(0, 0), (33, 0)], 64, 32)
    with pytest.raises(TypeError):
        ops.sw_gather_labels(lab.to(dev)[:, :, :2], [(0, 0)], 64, 32)        # not [H, W, 3]
    with pytest.raises(TypeError):
        ops.sw_gather_labels(lab.to(dev).transpose(0, 1), [(0, 0)], 64, 32)  # not contiguous
    with pytest.raises(TypeError):
        ops.sw_gather_labels(lab.to(dev).float(), [(0, 0)], 64, 32)
    planes = torch.zeros(3, 8, 8, dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.sw_mask_counts(planes, planes.cpu())
    with pytest.raises(TypeError):
        ops.sw_mask_counts(planes, planes[:2])
    with pytest.raises(TypeError):
        ops.sw_mask_counts(planes, planes, out=torch.zeros(3, 3, dtype=torch.int32, device=dev))
    h, w, p_size, size = E2E
    img, lab2 = _e2e_pair()
    with pytest.raises(ValueError, match='label'):
        A.segment_image(model, img, cfg(p_size, size), label_bgr=lab2[:-1])  # a label of another shape
    with pytest.raises(ValueError, match='label'):
        A.evaluate_image(model, img, lab2[:, :-1], cfg(p_size, size))
