"""Confidence maps on the device (csrc/sw_scores.hip) against the host functions they restate:
`ops.sw_merge_scores` against `patch_merge_scores` (the 255 merges written out in numpy), its level-127 mask against
`ops.sw_merge_masks`, its mask mode against `S > level`, `ops.sw_score_hist` against `score_hist`, and the new keywords of
`segment_image` / `evaluate_image` / `evaluate_images`.  Every value is an integer: every comparison is `np.array_equal`.
The cases are those of tests/test_sw_scores_host.py, whose rehearsal shows on the host that they can tell a wrong kernel from a
right one."""
import numpy as np
import pytest
import torch

from test_sliding_window_gpu import E2E, _image, _to_dev, model  # noqa: F401  (model: the seeded UNet_R_SS_v2 fixture)
from test_sw_labels_gpu import _planes
from test_sw_labels_host import cfg, label_image
from test_sw_scores_host import GEOMS, SEED, case, oracle


@pytest.mark.gpu
@pytest.mark.parametrize('classes', [1, 3])
@pytest.mark.parametrize('weighted', [False, True], ids=['unit', 'unique'])
@pytest.mark.parametrize('geom', GEOMS, ids=str)
def test_scores_equal_the_255_host_merges_and_masks_are_scores_above_the_level(pkg, dev, geom, weighted, classes):
    A, ops = pkg.aerial_image_segmentation_api, pkg.ops
    h, w, p_size, size, overlap = geom
    org, wts, probs, _ = case(A, geom, weighted)
    want = oracle(A, geom, weighted)[:classes]
    dprobs = _to_dev(ops, np.ascontiguousarray(probs[:, :classes]), dev)
    got = ops.sw_merge_scores(dprobs, org, wts, p_size, h, w)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (classes, h, w) and got.is_cuda
    got = got.cpu().numpy()
    for c in range(classes):
        assert len(np.unique(want[c])) >= 64, 'class %d of the expected scores is nearly constant: the case tests nothing' % c
    assert np.array_equal(got, want), 'differs at %d score bytes' % int((got != want).sum())
    # level 127 is today's kernel
    masks = ops.sw_merge_masks(dprobs, org, wts, p_size, h, w).cpu().numpy()
    assert np.array_equal(np.where(got > 127, 255, 0).astype(np.uint8), masks)
    assert np.array_equal(ops.sw_merge_scores(dprobs, org, wts, p_size, h, w, thresholds=127).cpu().numpy(), masks)
    # mask mode at the ends and the middle of the level range, per class
    for levels in ((0, 127, 254), (254, 0, 63), (200, 200, 200)):
        lv = list(levels[:classes])
        m = ops.sw_merge_scores(dprobs, org, wts, p_size, h, w, thresholds=lv if classes > 1 else lv[0]).cpu().numpy()
        assert m.dtype == np.uint8 and m.shape == (classes, h, w)
        for c in range(classes):
            assert np.array_equal(m[c], np.where(want[c] > lv[c], 255, 0).astype(np.uint8)), (levels, c)
    assert int(want.min()) <= 63 and int(want.max()) > 127                   # the levels 63 and 127 cut through every case's scores


# (classes, H * W, byte offsets of the score and ground-truth planes): as test_mask_counts_equal_numpy -- 5250 = 70 * 75 is no
# multiple of 16, equal offsets take 16 bytes per thread between a byte head and tail, unequal ones go byte by byte, an odd first
# byte, 131229 pixels spread over 3 blocks
@pytest.mark.gpu
@pytest.mark.parametrize('flat', [False, True], ids=['random', 'flat'])
@pytest.mark.parametrize('classes,hw,offs', [(3, 5250, (1, 1)), (3, 5250, (3, 5)), (3, 5250, (0, 0)), (1, 37, (7, 7)), (1, 37, (0, 9)),
                                              (3, 65536 * 2 + 157, (13, 13)), (2, 65536 * 2 + 157, (0, 4))])
def test_score_hist_equals_numpy(pkg, dev, classes, hw, offs, flat):
    A, ops = pkg.aerial_image_segmentation_api, pkg.ops
    sc, hs = _planes(classes, hw, offs[0], 61, dev)
    gt, hg = _planes(classes, hw, offs[1], 62, dev)
    if flat:                                                                 # runs of one value, as a confident model gives: 0, 255, a ramp
        hs = np.repeat(np.array([0, 255, 0, 254, 255, 1, 255], dtype=np.uint8), -(-hw // 7))[:hw][None].repeat(classes, 0)
        hs = np.ascontiguousarray(np.roll(hs, 3, 1))
        sc.copy_(torch.from_numpy(hs))
    want = A.score_hist(hs, hg)
    assert want.shape == (classes, 2, 256) and (want.sum((1, 2)) == hw).all() and (want[:, 0].sum(1) > 0).all() and (want[:, 1].sum(1) > 0).all()
    got = ops.sw_score_hist(sc, gt)
    assert got.dtype == torch.int64 and tuple(got.shape) == (classes, 2, 256) and got.is_cuda
    assert np.array_equal(got.cpu().numpy(), want)
    again = ops.sw_score_hist(sc, gt, out=got)                               # accumulates
    assert again is got and np.array_equal(got.cpu().numpy(), 2 * want)
    if hw == 5250:                                                           # [C, H, W] as the merge leaves it
        assert np.array_equal(ops.sw_score_hist(sc.view(classes, 70, 75), gt.view(classes, 70, 75)).cpu().numpy(), want)
    # the counts of sw_mask_counts are the suffix sums at level 127
    counts = ops.sw_mask_counts(sc, gt).cpu().numpy()
    assert np.array_equal(counts, np.stack([want[:, 1, 128:].sum(1), want[:, :, 128:].sum((1, 2)), want[:, 1].sum(1)], 1))


def _e2e_pair(seed=22, block=3):
    h, w, p_size, size = E2E
    return _image(h, w, seed), label_image(h, w, block, SEED + 10 + seed)


@pytest.mark.gpu
def test_segment_image_threshold_and_scores(pkg, dev, model):
    A = pkg.aerial_image_segmentation_api
    h, w, p_size, size = E2E
    cfg_, (img, lab) = cfg(p_size, size), _e2e_pair()
    base = A.segment_image(model, img, cfg_, batch_size=6)
    at127 = A.segment_image(model, img, cfg_, batch_size=6, threshold=127)
    assert isinstance(at127, list) and all(np.array_equal(a, b) for a, b in zip(at127, base))
    # the scores are the host oracle of the probabilities that were merged, and every mask is a cut through them
    res = A.segment_image(model, img, cfg_, batch_size=6, return_probs=True, return_scores=True)
    assert len(res) == 5
    masks, probs, org, wts, scores = res
    full = A.patch_origins(h, w, p_size, 0.5)
    want = A.patch_merge_scores(img, [probs[org.index(o)] for o in full], p_size, cfg_, 0.5)
    assert len(scores) == 3 and all(s.dtype == np.uint8 and s.shape == (h, w) for s in scores)
    assert all(np.array_equal(a, b) for a, b in zip(scores, want))
    assert all(np.array_equal(m, b) for m, b in zip(masks, base))
    levels = (3, 127, 250)
    cut = A.segment_image(model, img, cfg_, batch_size=6, threshold=levels)
    assert all(np.array_equal(m, np.where(s > t, 255, 0).astype(np.uint8)) for m, s, t in zip(cut, scores, levels))
    assert not all(np.array_equal(a, b) for a, b in zip(cut, base))
    one, all24 = A.segment_image(model, img, cfg_, batch_size=6, threshold=90, dedupe=False, return_scores=True)
    assert all(np.array_equal(m, np.where(s > 90, 255, 0).astype(np.uint8)) for m, s in zip(one, all24))
    # with test-time augmentation and a label: (masks, gt, probs, origins, weights, scores)
    res = A.segment_image(model, img, cfg_, batch_size=6, tta='hflip', label_bgr=lab, return_probs=True, return_scores=True, threshold=100)
    assert len(res) == 6
    masks, gt, probs, org, wts, scores = res
    _, gt0 = A.segment_image(model, img, cfg_, batch_size=6, label_bgr=lab)
    assert all(np.array_equal(a, b) for a, b in zip(gt, gt0))                # the ground truth depends on neither keyword
    want = A.patch_merge_scores(img, [probs[org.index(o)] for o in full], p_size, cfg_, 0.5)
    assert all(np.array_equal(a, b) for a, b in zip(scores, want))
    assert all(np.array_equal(m, np.where(s > 100, 255, 0).astype(np.uint8)) for m, s in zip(masks, scores))
    plain = A.segment_image(model, img, cfg_, batch_size=6, tta='hflip')
    assert all(np.array_equal(p, np.where(s > 127, 255, 0).astype(np.uint8)) for p, s in zip(plain, scores))
    only = A.segment_image(model, img, cfg_, batch_size=6, tta='hflip', return_scores=True)
    assert isinstance(only, tuple) and len(only) == 2 and all(np.array_equal(a, b) for a, b in zip(only[1], scores))
    for bad in (True, 255, -1, 1.0, (0, 127), (0, 127, 255)):
        with pytest.raises(ValueError, match='threshold'):
            A.segment_image(model, img, cfg_, threshold=bad)


@pytest.mark.gpu
def test_evaluate_images_sweep(pkg, dev, model):
    A, ops = pkg.aerial_image_segmentation_api, pkg.ops
    h, w, p_size, size = E2E
    cfg_ = cfg(p_size, size)
    pairs = [_e2e_pair(22, 3), _e2e_pair(23, 5)]
    plain = A.evaluate_images(model, pairs, cfg_, batch_size=6)
    res = A.evaluate_images(model, pairs, cfg_, batch_size=6, sweep=True)
    assert sorted(plain) == ['counts', 'dice', 'iou']
    assert sorted(res) == ['best_iou', 'best_threshold', 'counts', 'dice', 'dice_curve', 'hist', 'iou', 'iou_curve']
    assert np.array_equal(res['counts'], plain['counts']) and res['iou'] == plain['iou'] and res['dice'] == plain['dice']
    want = np.zeros((3, 2, 256), dtype=np.int64)
    for img, lab in pairs:
        _, gt, scores = A.segment_image(model, img, cfg_, batch_size=6, label_bgr=lab, return_scores=True)
        want += A.score_hist(scores, gt)
    assert isinstance(res['hist'], np.ndarray) and res['hist'].dtype == np.int64 and np.array_equal(res['hist'], want)
    assert want.sum() == 2 * 3 * h * w and (want[:, 1].sum(1) > 0).all()
    curves = A.threshold_curves(want)
    assert np.array_equal(res['iou_curve'], curves['iou_curve']) and np.array_equal(res['dice_curve'], curves['dice_curve'])
    assert res['best_threshold'] == curves['best_threshold'] and res['best_iou'] == curves['best_iou']
    for c in range(3):                                                       # the curves pass through the level-127 numbers
        assert res['iou_curve'][c, 127] == res['iou'][c] and res['dice_curve'][c, 127] == res['dice'][c]
        assert res['best_iou'][c] == res['iou_curve'][c].max() >= res['iou'][c]
    # evaluate_image: True starts a histogram, a tensor accumulates, counts still fill
    img, lab = pairs[0]
    h0 = A.evaluate_image(model, img, lab, cfg_, batch_size=6, hist=True)
    assert h0.is_cuda and h0.dtype == torch.int64 and tuple(h0.shape) == (3, 2, 256)
    counts = torch.zeros((3, 3), dtype=torch.int64, device=dev)
    h1 = A.evaluate_image(model, pairs[1][0], pairs[1][1], cfg_, batch_size=6, counts=counts, hist=h0)
    assert h1 is h0 and np.array_equal(h0.cpu().numpy(), want)
    assert np.array_equal(counts.cpu().numpy(), A.evaluate_image(model, pairs[1][0], pairs[1][1], cfg_, batch_size=6).cpu().numpy())
    with pytest.raises(TypeError, match='hist'):
        A.evaluate_image(model, img, lab, cfg_, hist=torch.zeros((3, 2, 256), dtype=torch.int32, device=dev))
    with pytest.raises(TypeError):
        ops.sw_score_hist(torch.zeros(3, 8, 8, dtype=torch.uint8, device=dev), torch.zeros(3, 8, 8, dtype=torch.uint8, device=dev),
                          out=torch.zeros((3, 256), dtype=torch.int64, device=dev))
