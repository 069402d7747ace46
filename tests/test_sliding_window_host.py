"""CPU: the host half of device-side sliding-window inference -- `unique_origins`, the weighted form of `patch_merge`'s
overlap vote that the merge kernel computes, and the two C-ABI entries' argument checks (which run before any launch)."""
import ctypes

import numpy as np
import pytest


def test_unique_origins_shipped_geometry_9_origins_4_times_each(pkg):
    A = pkg.aerial_image_segmentation_api
    org = A.patch_origins(2048, 2048, 1024, 0.5)
    uniq, mult = A.unique_origins(org)
    assert len(org) == 36 and len(uniq) == 9 and mult == [4] * 9
    first = []
    for o in org:
        if o not in first:
            first.append(o)
    assert uniq == first and uniq[0] == (0, 0) and uniq[1] == (512, 0)     # first-appearance order: the top-left sweep's own
    assert set(uniq) == {(h, w) for h in (0, 512, 1024) for w in (0, 512, 1024)}


def test_unique_origins_non_coinciding_sweeps_stay_36(pkg):
    A = pkg.aerial_image_segmentation_api
    org = A.patch_origins(70, 75, 32, 0.5)
    uniq, mult = A.unique_origins(org)
    assert len(org) == 36 and uniq == org and mult == [1] * 36              # 3 x 3 positions per sweep, four distinct sweeps
    assert {h for h, _ in org} == {0, 16, 32, 38, 22, 6} and {w for _, w in org} == {0, 16, 32, 43, 27, 11}


@pytest.mark.parametrize('hw,p_size', [((96, 96), 64), ((2048 // 16, 2048 // 16), 1024 // 16), ((70, 75), 32)])
def test_weighted_vote_over_unique_origins_equals_patch_merge_over_the_full_list(pkg, hw, p_size):
    """k = sum of weight * [map is 1], n = sum of weights over the unique origins, (int)(k / n * 255) > 127 -- what the merge
    kernel evaluates -- against `patch_merge` accumulating every duplicate on its own, for random {0, 1} maps."""
    A = pkg.aerial_image_segmentation_api
    h, w = hw
    org = A.patch_origins(h, w, p_size, 0.5)
    uniq, mult = A.unique_origins(org)
    rng = np.random.default_rng(11)
    maps = {o: (rng.random((2, p_size, p_size)) < 0.5).astype(np.float32) for o in uniq}
    want = A.patch_merge(np.zeros((h, w, 3), np.uint8), [maps[o] for o in org], p_size, dict(num_classes=2), 0.5)
    k = np.zeros((2, h, w), np.int64); n = np.zeros((h, w), np.int64)
    for (h1, w1), m in zip(uniq, mult):
        k[:, h1:h1 + p_size, w1:w1 + p_size] += m * maps[(h1, w1)].astype(np.int64)
        n[h1:h1 + p_size, w1:w1 + p_size] += m
    n[n == 0] = 1
    got = np.where((k.astype(np.float64) / n.astype(np.float64) * 255.0).astype(np.int64) > 127, 255, 0).astype(np.uint8)
    assert np.array_equal(got, np.stack(want))
    assert set(np.unique(got)) == {0, 255}
    # the integer form of the final threshold, for every vote that can occur with up to 16 covering patches
    for nn in range(1, 17):
        for kk in range(nn + 1):
            assert (int(float(kk) / float(nn) * 255.0) > 127) == (255 * kk >= 128 * nn), (kk, nn)


def test_sliding_window_entries_refuse_bad_arguments_without_a_launch(pkg):
    """Null pointers, a resize factor of 3 and a patch outside the image: a status and a message, from the host side of the
    entry -- safe without a GPU (the pointers that stand for device memory are never dereferenced)."""
    lib = pkg._lib
    L = lib.load()
    fake = ctypes.c_void_p(4096)                                             # stands for device memory
    org = (ctypes.c_int32 * 2)(0, 0)
    consts = [0.0] * 6
    assert L.ssg_sw_gather_patches_u8_f32(None, 96, 96, None, None, 1, 64, 32, *(consts + [None, None])) != 0
    assert b'sw_gather' in L.ssg_last_error()
    assert L.ssg_sw_gather_patches_u8_f32(fake, 96, 96, fake, org, 1, 48, 16, *(consts + [fake, None])) != 0
    assert b'sw_gather' in L.ssg_last_error() and b'factors 1 and 2' in L.ssg_last_error()
    assert L.ssg_sw_gather_patches_u8_f32(fake, 96, 96, fake, org, 0, 64, 32, *(consts + [fake, None])) != 0
    out_org = (ctypes.c_int32 * 2)(33, 0)
    assert L.ssg_sw_gather_patches_u8_f32(fake, 96, 96, fake, out_org, 1, 64, 32, *(consts + [fake, None])) != 0
    assert b'outside' in L.ssg_last_error()
    assert L.ssg_sw_merge_masks_f32_u8(None, 4, 1, 3, 32, None, None, None, 64, 96, 96, None, None) != 0
    assert b'sw_merge' in L.ssg_last_error()
    assert L.ssg_sw_merge_masks_f32_u8(fake, 4, 1, 3, 16, fake, org, fake, 48, 96, 96, fake, None) != 0
    assert b'sw_merge' in L.ssg_last_error() and b'factors 1 and 2' in L.ssg_last_error()
    assert L.ssg_sw_merge_masks_f32_u8(fake, 4, 1, 3, 32, fake, out_org, fake, 64, 96, 96, fake, None) != 0
    assert b'outside' in L.ssg_last_error()
    with pytest.raises(RuntimeError, match='ssg_sw_gather_patches_u8_f32 failed'):
        lib.call('ssg_sw_gather_patches_u8_f32', fake, 96, 96, fake, org, 1, 48, 16, *(consts + [fake, None]))


def test_wrappers_refuse_cpu_tensors(pkg):
    import torch
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        pkg.ops.sw_gather_patches(torch.zeros(96, 96, 3, dtype=torch.uint8), [(0, 0)], 64, 32)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        pkg.ops.sw_merge_masks(torch.zeros(1, 3, 32, 32), [(0, 0)], [1], 64, 96, 96)
