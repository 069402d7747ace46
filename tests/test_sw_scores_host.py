"""CPU: the host half of the confidence maps -- the argument checks of the two C-ABI entries
(`ssg_sw_merge_scores_f32_u8`, `ssg_sw_score_hist_u8`), which run before any launch; the host oracle `patch_merge_scores` against
`patch_merge`; the curve arithmetic of `evaluate_images(sweep=True)`; and a rehearsal on the host showing that the inputs of
tests/test_sw_scores_gpu.py can tell a right kernel from a wrong one."""
import ctypes
import inspect

import numpy as np
import pytest

# (image H, W, patch, inference size, overlap): 70 x 75 puts origins at odd byte offsets, at both factors; a 300-pixel row spans
# two 256-pixel blocks; 40 x 44 at patch 8, overlap 0.75 has 1292 patches (21 list refills) and up to 64 of them on a pixel
GEOMS = [(70, 75, 32, 16, 0.5), (70, 75, 32, 32, 0.5), (72, 300, 64, 32, 0.5), (40, 44, 8, 4, 0.75)]
SEED = 2700


def score_probs(n, c, s, seed):
    """[n, c, s, s] float32 in [0, 1]: 40 % uniform, 20 % exactly float32(k / 255), 15 % each that value one ulp up / down,
    5 % each exact 0 and 1."""
    rng = np.random.default_rng(seed)
    shape = (n, c, s, s)
    kind = rng.choice(6, size=shape, p=(.4, .2, .15, .15, .05, .05))
    lv = (rng.integers(0, 256, shape).astype(np.float32) / np.float32(255)).astype(np.float32)
    p = rng.random(shape, dtype=np.float32)
    p = np.where(kind == 1, lv, p)
    p = np.where(kind == 2, np.nextafter(lv, np.float32(2)), p)
    p = np.where(kind == 3, np.nextafter(lv, np.float32(-1)), p)
    p = np.where(kind == 4, np.float32(0), p)
    p = np.where(kind == 5, np.float32(1), p)
    return np.clip(p, 0, 1).astype(np.float32)


def case(A, geom, weighted, seed=SEED):
    """(origins, weights, probabilities [P', 3, s, s] for the device, the full-length patch list for the host oracle)."""
    h, w, p_size, size, overlap = geom
    full = A.patch_origins(h, w, p_size, overlap)
    if not weighted:
        probs = score_probs(len(full), 3, size, seed + GEOMS.index(geom))
        return full, [1] * len(full), probs, list(probs)
    uniq, mult = A.unique_origins(full)
    probs = score_probs(len(uniq), 3, size, seed + 50 + GEOMS.index(geom))
    where = {o: i for i, o in enumerate(uniq)}
    return uniq, mult, probs, [probs[where[o]] for o in full]


def kernel_scores(org, wts, probs, p_size, h, w, tie_wins=False, round_add=8, clamp=True):
    """sw_merge_scores_kernel restated in integers on the host: r = (uint8)(p * 255), at factor 2 (9a + 3b + 3c + d + 8) >> 4
    over edge-clamped taps; per pixel the weighted count of every r value, k(L) = weight with r >= L, and S = the largest
    L in 1 .. 255 with (int)(k / n * 255.0) > 127.  The keywords restate three mistakes a kernel could make."""
    n_p, classes, s, _ = probs.shape
    u8 = (probs * 255).astype(np.uint8).astype(np.int64)
    if p_size == s:
        r = u8
    else:
        def nb(a, axis, d):
            if not clamp:
                return np.roll(a, -d, axis)                                  # the neighbour in memory, whatever it belongs to
            idx = np.clip(np.arange(s) + d, 0, s - 1)
            return np.take(a, idx, axis)
        r = np.empty((n_p, classes, p_size, p_size), dtype=np.int64)
        for py, dy in ((0, -1), (1, 1)):
            for px, dx in ((0, -1), (1, 1)):
                a, b, c, d = u8, nb(u8, 3, dx), nb(u8, 2, dy), nb(nb(u8, 2, dy), 3, dx)
                r[:, :, py::2, px::2] = (9 * a + 3 * b + 3 * c + d + round_add) >> 4
    cnt = np.zeros((classes, 256, h, w), dtype=np.int64)
    n = np.zeros((h, w), dtype=np.int64)
    yy, xx = np.mgrid[0:p_size, 0:p_size]
    for (h1, w1), m, rp in zip(org, wts, r):
        for c in range(classes):
            np.add.at(cnt[c], (rp[c], h1 + yy, w1 + xx), m)
        n[h1:h1 + p_size, w1:w1 + p_size] += m
    k = np.cumsum(cnt[:, ::-1], axis=1)[:, ::-1]                             # k[c, L]: weight of the voters with r >= L
    dn = np.where(n == 0, 1, n)
    if tie_wins:
        on = 2 * k >= dn
    else:
        on = (k.astype(np.float64) / dn.astype(np.float64) * 255.0).astype(np.int64) > 127
    on[:, 0] = False
    on &= (n > 0)
    levels = np.arange(256).reshape(1, 256, 1, 1)
    return np.where(on, levels, 0).max(1).astype(np.uint8)


_ORACLE = {}


def oracle(A, geom, weighted):
    """[3, H, W] uint8: `patch_merge_scores` of the case, computed once per session."""
    key = (geom, weighted)
    if key not in _ORACLE:
        h, w, p_size, size, overlap = geom
        _, _, _, full = case(A, geom, weighted)
        _ORACLE[key] = np.stack(A.patch_merge_scores(np.zeros((h, w, 3), np.uint8), full, p_size, dict(num_classes=3), overlap))
        _ORACLE[key].setflags(write=False)
    return _ORACLE[key]


def test_score_entries_refuse_bad_arguments_without_a_launch(pkg):
    lib = pkg._lib
    L = lib.load()
    fake = ctypes.c_void_p(4096)                                             # stands for device memory: never dereferenced
    org = (ctypes.c_int32 * 2)(0, 0)
    lv = (ctypes.c_int32 * 3)(0, 127, 254)
    merge = L.ssg_sw_merge_scores_f32_u8

    def refused(rc, *words):
        msg = L.ssg_last_error()
        assert rc != 0 and all(w in msg for w in words), (rc, msg)

    refused(merge(None, 4, 1, 3, 32, None, None, None, 64, 96, 96, None, None, None), b'sw_merge_scores', b'null')
    refused(merge(fake, 4, 1, 3, 32, fake, None, fake, 64, 96, 96, None, fake, None), b'sw_merge_scores', b'null')
    refused(merge(fake, 4, 1, 3, 32, fake, org, None, 64, 96, 96, lv, fake, None), b'sw_merge_scores', b'null')
    refused(merge(fake, 4, 1, 3, 32, fake, org, fake, 64, 96, 96, lv, None, None), b'sw_merge_scores', b'null')
    refused(merge(fake, 4, 0, 3, 32, fake, org, fake, 64, 96, 96, None, fake, None), b'sw_merge_scores', b'P 0')
    refused(merge(fake, 4, -2, 3, 32, fake, org, fake, 64, 96, 96, lv, fake, None), b'sw_merge_scores', b'P -2')
    refused(merge(fake, 4, 1, 3, 16, fake, org, fake, 48, 96, 96, None, fake, None), b'sw_merge_scores', b'factors 1 and 2')
    refused(merge(fake, 4, 1, 3, 16, fake, org, fake, 64, 96, 96, lv, fake, None), b'sw_merge_scores', b'factors 1 and 2')
    out_org = (ctypes.c_int32 * 2)(33, 0)
    refused(merge(fake, 4, 1, 3, 32, fake, out_org, fake, 64, 96, 96, None, fake, None), b'sw_merge_scores', b'outside')
    neg_org = (ctypes.c_int32 * 4)(0, 0, 0, -1)
    refused(merge(fake, 4, 2, 3, 32, fake, neg_org, fake, 64, 96, 96, lv, fake, None), b'sw_merge_scores', b'outside')
    for bad in (255, -1, 1000):
        refused(merge(fake, 4, 1, 3, 32, fake, org, fake, 64, 96, 96, (ctypes.c_int32 * 3)(0, 127, bad), fake, None),
                b'sw_merge_scores', b'level %d' % bad, b'0 .. 254')
    refused(merge(fake, 4, 1, 5, 32, fake, org, fake, 64, 96, 96, None, fake, None), b'sw_merge_scores', b'ld 4')

    hist = L.ssg_sw_score_hist_u8
    refused(hist(None, None, 3, 100, None, None), b'sw_score_hist', b'null')
    refused(hist(fake, None, 3, 100, fake, None), b'sw_score_hist', b'null')
    refused(hist(fake, fake, 3, 100, None, None), b'sw_score_hist', b'null')
    refused(hist(fake, fake, 0, 100, fake, None), b'sw_score_hist', b'0 classes')
    refused(hist(fake, fake, 3, 0, fake, None), b'sw_score_hist', b'0 pixels')
    refused(hist(fake, fake, 3, 100, ctypes.c_void_p(4100), None), b'sw_score_hist', b'aligned')
    with pytest.raises(RuntimeError, match='ssg_sw_merge_scores_f32_u8 failed'):
        lib.call('ssg_sw_merge_scores_f32_u8', fake, 4, 1, 3, 32, fake, org, fake, 64, 96, 96, (ctypes.c_int32 * 3)(0, 0, 255), fake, None)
    with pytest.raises(RuntimeError, match='ssg_sw_score_hist_u8 failed'):
        lib.call('ssg_sw_score_hist_u8', fake, fake, 0, 100, fake, None)
    assert L.ssg_abi_version() == 10                                         # additive: no layout changed


def test_score_wrappers_check_before_any_launch(pkg):
    import torch
    A, ops = pkg.aerial_image_segmentation_api, pkg.ops
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.sw_merge_scores(torch.zeros(1, 3, 16, 16), [(0, 0)], [1], 32, 96, 96)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.sw_score_hist(torch.zeros(3, 8, 8, dtype=torch.uint8), torch.zeros(3, 8, 8, dtype=torch.uint8))
    assert ops.sw_levels(5, 3) == [5, 5, 5] and ops.sw_levels((0, 127, 254), 3) == [0, 127, 254] and ops.sw_levels([7], 1) == [7]
    cfg = dict(patch_size=64, input_w=32, input_h=32, patch_overlap=0.5, num_classes=3)
    for bad in (True, False, 255, -1, 1.0, '127', (0, 127), (0, 127, 255), (0, True, 3), [1.5, 2, 3], np.int64(3)):
        with pytest.raises(ValueError, match='threshold'):
            ops.sw_levels(bad, 3)
        with pytest.raises(ValueError, match='threshold'):                   # before the first upload: there is no model and no image
            A.segment_image(None, None, cfg, threshold=bad)
    with pytest.raises(TypeError, match='hist'):
        A.evaluate_image(None, None, np.zeros((8, 8, 3), np.uint8), cfg, hist=np.zeros((3, 2, 256), np.int64))
    for fn, name, default in ((A.segment_image, 'threshold', None), (A.segment_image, 'return_scores', False),
                              (A.evaluate_image, 'hist', None), (A.evaluate_images, 'sweep', False)):
        assert inspect.signature(fn).parameters[name].default is default
    assert inspect.signature(ops.sw_merge_scores).parameters['thresholds'].default is None
    assert list(inspect.signature(ops.sw_score_hist).parameters) == ['scores', 'gt', 'out']


@pytest.mark.parametrize('weighted', [False, True], ids=['unit', 'unique'])
@pytest.mark.parametrize('geom', GEOMS, ids=str)
def test_scores_above_127_are_patch_merge_and_the_restated_kernel_is_the_oracle(pkg, geom, weighted):
    A = pkg.aerial_image_segmentation_api
    h, w, p_size, size, overlap = geom
    org, wts, probs, full = case(A, geom, weighted)
    want = oracle(A, geom, weighted)
    masks = np.stack(A.patch_merge(np.zeros((h, w, 3), np.uint8), full, p_size, dict(num_classes=3), overlap))
    assert want.dtype == np.uint8 and want.shape == masks.shape == (3, h, w)
    assert np.array_equal(np.where(want > 127, 255, 0).astype(np.uint8), masks)
    for c in range(3):
        assert set(np.unique(masks[c])) == {0, 255} and len(np.unique(want[c])) >= 64, (c, len(np.unique(want[c])))
    assert np.array_equal(kernel_scores(org, wts, probs, p_size, h, w), want)


@pytest.mark.parametrize('weighted', [False, True], ids=['unit', 'unique'])
@pytest.mark.parametrize('geom', GEOMS, ids=str)
def test_rehearsal_the_score_cases_can_fail(pkg, geom, weighted):
    """Three mistakes restated on the host, each against the oracle: a tie that wins the vote (k / n >= 0.5, where patch_merge's
    (int)(k / n * 255.0) > 127 needs k / n >= 128 / 255), + 7 instead of + 8 in the x2 rounding, and edge taps that are not
    clamped.  Each must change score bytes -- the last two wherever the x2 resize runs: at factor 1 there is no rounding and no
    tap, the restated kernel does not take that path, and the two mistakes must then change nothing."""
    A = pkg.aerial_image_segmentation_api
    h, w, p_size, size, overlap = geom
    org, wts, probs, _ = case(A, geom, weighted)
    want = oracle(A, geom, weighted)
    diff = {name: int((kernel_scores(org, wts, probs, p_size, h, w, **kw) != want).sum())
            for name, kw in (('tie wins', dict(tie_wins=True)), ('+7', dict(round_add=7)), ('unclamped', dict(clamp=False)))}
    print(geom, 'weighted' if weighted else 'unit', 'score bytes changed:', diff)
    assert diff['tie wins'] >= 1
    if p_size == size:
        assert diff['+7'] == 0 and diff['unclamped'] == 0
    else:
        assert diff['+7'] >= 1 and diff['unclamped'] >= 1


def test_score_hist_is_a_bincount(pkg):
    A = pkg.aerial_image_segmentation_api
    rng = np.random.default_rng(SEED)
    s = rng.integers(0, 256, (2, 9, 11), dtype=np.uint8)
    g = rng.integers(0, 256, (2, 9, 11), dtype=np.uint8)
    got = A.score_hist(s, g)
    assert got.dtype == np.int64 and got.shape == (2, 2, 256) and got.sum() == s.size
    for c in range(2):
        for bit in range(2):
            for v in (0, 1, 127, 128, 255):
                assert got[c, bit, v] == int(((s[c] == v) & ((g[c] > 127) == bool(bit))).sum())
    assert np.array_equal(A.score_hist(list(s), list(g)), got)


def test_threshold_curves_from_a_hand_made_histogram(pkg):
    A = pkg.aerial_image_segmentation_api
    hist = np.zeros((2, 2, 256), dtype=np.int64)
    # class 0: background scores 0 (50 px) and 100 (10 px), ground truth scores 100 (5 px), 200 (30 px) and 255 (5 px)
    hist[0, 0, 0], hist[0, 0, 100], hist[0, 1, 100], hist[0, 1, 200], hist[0, 1, 255] = 50, 10, 5, 30, 5
    # class 1: nothing is ground truth, 7 px at score 255
    hist[1, 0, 255] = 7
    res = A.threshold_curves(hist)
    iou, dice = res['iou_curve'], res['dice_curve']
    assert iou.shape == dice.shape == (2, 255) and iou.dtype == np.float64
    e = 1e-5
    for t, (i, p) in ((0, (40, 50)), (99, (40, 50)), (100, (35, 35)), (127, (35, 35)), (199, (35, 35)), (200, (5, 5)), (254, (5, 5))):
        assert iou[0, t] == (i + e) / (p + 40 - i + e), t
        assert dice[0, t] == (2 * i + e) / (p + 40 + e), t
    assert np.all(iou[1] == e / (7 + e)) and np.all(dice[1] == e / (7 + e))
    assert res['best_threshold'] == [100, 0] and res['best_iou'] == [float(iou[0, 100]), float(iou[1, 0])]   # lowest level on ties
    assert all(isinstance(v, int) for v in res['best_threshold']) and all(isinstance(v, float) for v in res['best_iou'])
    # level 127 of the curves is what evaluate_images computes from the counts (I, P, G)
    i, p, g = 35, 35, 40
    assert iou[0, 127] == float((i + e) / (p + g - i + e)) and dice[0, 127] == float((2 * i + e) / (p + g + e))
    with pytest.raises(ValueError):
        A.threshold_curves(np.zeros((2, 256)))
