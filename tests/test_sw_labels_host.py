"""CPU: the host half of the device-side ground-truth branch -- the argument checks of the two C-ABI entries
(`ssg_sw_gather_labels_u8_f32`, `ssg_sw_mask_counts_u8`), which run before any launch, and a rehearsal on the host functions
showing that the label images of tests/test_sw_labels_gpu.py can tell a right kernel from a wrong one."""
import ctypes

import numpy as np
import pytest

# (image H, W, patch, inference size) of tests/test_sliding_window_gpu.py: 70 x 75 puts origins at odd byte offsets
GEOMS = [(70, 75, 32, 16), (70, 75, 32, 32), (96, 96, 64, 32)]
# the three palette entries of mask_convert, a colour of no class, and two near-misses of classes 0 and 1
COLOURS = np.array([(255, 255, 255), (255, 0, 0), (0, 0, 255), (0, 255, 0), (254, 255, 255), (255, 0, 1)], dtype=np.uint8)
COLOUR_P = (.3, .25, .25, .1, .05, .05)
BLOCKS = (1, 2, 3, 5)
SEED = 400


def label_image(h, w, block, seed):
    """[h, w, 3] uint8: i.i.d. colours of COLOURS with COLOUR_P, constant over block x block pixels."""
    rng = np.random.default_rng(seed)
    idx = rng.choice(len(COLOURS), size=(-(-h // block), -(-w // block)), p=COLOUR_P)
    idx = np.repeat(np.repeat(idx, block, 0), block, 1)[:h, :w]
    return np.ascontiguousarray(COLOURS[idx])


def cfg(p_size, size, classes=3):
    return dict(patch_size=p_size, input_w=size, input_h=size, patch_overlap=0.5, num_classes=classes)


def host_labels(A, lab, p_size, size, classes):
    """[P, classes, size, size] float64 in {0, 1}: the gt_label list of segmentation_inference_full."""
    _, patches = A.patch_gen(lab, lab, p_size, 0.5)
    return np.stack([np.stack([A.mask_convert(p, c, size) for c in range(classes)]) / 255.0 for p in patches])


def host_gt_masks(A, lab, p_size, size, classes):
    return np.stack(A.patch_merge(lab, list(host_labels(A, lab, p_size, size, classes)), p_size, dict(num_classes=classes), 0.5))


def pixel_masks(lab, classes=3):
    """The class masks taken pixel by pixel at image resolution: [classes, H, W] uint8 in {0, 255}."""
    return np.stack([np.where((lab == COLOURS[c]).all(-1), 255, 0).astype(np.uint8) for c in range(classes)])


def test_label_entries_refuse_bad_arguments_without_a_launch(pkg):
    lib = pkg._lib
    L = lib.load()
    fake = ctypes.c_void_p(4096)                                             # stands for device memory: never dereferenced
    org = (ctypes.c_int32 * 2)(0, 0)
    gather = L.ssg_sw_gather_labels_u8_f32

    def refused(rc, *words):
        msg = L.ssg_last_error()
        assert rc != 0 and all(w in msg for w in words), (rc, msg)

    refused(gather(None, 96, 96, None, None, 1, 64, 32, 3, None, None), b'sw_gather_labels', b'null')
    refused(gather(fake, 96, 96, fake, None, 1, 64, 32, 3, fake, None), b'sw_gather_labels', b'null')
    refused(gather(fake, 96, 96, fake, org, 1, 48, 16, 3, fake, None), b'sw_gather_labels', b'factors 1 and 2')
    refused(gather(fake, 96, 96, fake, org, 0, 64, 32, 3, fake, None), b'sw_gather_labels', b'P 0')
    out_org = (ctypes.c_int32 * 2)(33, 0)
    refused(gather(fake, 96, 96, fake, out_org, 1, 64, 32, 3, fake, None), b'sw_gather_labels', b'outside')
    neg_org = (ctypes.c_int32 * 4)(0, 0, 0, -1)
    refused(gather(fake, 96, 96, fake, neg_org, 2, 64, 32, 3, fake, None), b'sw_gather_labels', b'outside')
    refused(gather(fake, 96, 96, fake, org, 1, 64, 32, 0, fake, None), b'sw_gather_labels', b'0 classes')
    refused(gather(fake, 96, 96, fake, org, 1, 64, 32, 4, fake, None), b'sw_gather_labels', b'4 classes')
    refused(gather(ctypes.c_void_p(4098), 96, 96, fake, org, 1, 64, 32, 3, fake, None), b'sw_gather_labels', b'aligned')
    refused(gather(fake, 96, 96, fake, org, 1, 64, 32, 3, ctypes.c_void_p(4100), None), b'sw_gather_labels', b'aligned')

    counts = L.ssg_sw_mask_counts_u8
    refused(counts(None, None, 3, 100, None, None), b'sw_mask_counts', b'null')
    refused(counts(fake, fake, 3, 100, None, None), b'sw_mask_counts', b'null')
    refused(counts(fake, None, 3, 100, fake, None), b'sw_mask_counts', b'null')
    refused(counts(fake, fake, 0, 100, fake, None), b'sw_mask_counts', b'0 classes')
    refused(counts(fake, fake, -1, 100, fake, None), b'sw_mask_counts')
    refused(counts(fake, fake, 3, 0, fake, None), b'sw_mask_counts', b'0 pixels')
    refused(counts(fake, fake, 3, 100, ctypes.c_void_p(4100), None), b'sw_mask_counts', b'aligned')
    with pytest.raises(RuntimeError, match='ssg_sw_gather_labels_u8_f32 failed'):
        lib.call('ssg_sw_gather_labels_u8_f32', fake, 96, 96, fake, org, 1, 64, 32, 4, fake, None)
    with pytest.raises(RuntimeError, match='ssg_sw_mask_counts_u8 failed'):
        lib.call('ssg_sw_mask_counts_u8', fake, fake, 0, 100, fake, None)
    assert L.ssg_abi_version() == 10                                         # additive: no layout changed


def test_label_wrappers_refuse_cpu_tensors(pkg):
    import torch
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        pkg.ops.sw_gather_labels(torch.zeros(96, 96, 3, dtype=torch.uint8), [(0, 0)], 64, 32)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        pkg.ops.sw_mask_counts(torch.zeros(3, 8, 8, dtype=torch.uint8), torch.zeros(3, 8, 8, dtype=torch.uint8))


def test_half_resolution_mask_is_at_least_two_of_the_box(pkg):
    """The integer identity of the factor-2 kernel: for every 2 x 2 box of a {0, 255} mask with k selected pixels,
    post_process_resized_mask(resize_u8(box, 1, 1)) is 255 exactly when k >= 2, through (255 k + 2) >> 2."""
    A = pkg.aerial_image_segmentation_api
    seen = set()
    for bits in range(16):
        box = np.array([255 if bits >> i & 1 else 0 for i in range(4)], dtype=np.uint8).reshape(2, 2)
        k = bin(bits).count('1')
        half = A.resize_u8(box, 1, 1)
        assert int(half[0, 0]) == (255 * k + 2) >> 2 == (0, 64, 128, 191, 255)[k]
        assert int(A.post_process_resized_mask(half)[0, 0]) == (255 if k >= 2 else 0)
        seen.add(k)
    assert seen == {0, 1, 2, 3, 4}


@pytest.mark.parametrize('block', BLOCKS)
@pytest.mark.parametrize('h,w,p_size,size', GEOMS)
def test_rehearsal_the_label_cases_can_fail(pkg, h, w, p_size, size, block):
    """On the host functions alone: the expected ground-truth masks are non-constant with a coverage near the colour
    probabilities; at factor 1 they are the per-pixel class masks, at factor 2 they are not -- a kernel that skipped the
    1/2 -> x2 round trip, or compared a colour loosely, would differ from them at hundreds of pixels."""
    A = pkg.aerial_image_segmentation_api
    lab = label_image(h, w, block, SEED + block)
    want = host_gt_masks(A, lab, p_size, size, 3)
    px = pixel_masks(lab)
    for c in range(3):
        assert set(np.unique(want[c])) == {0, 255}
        assert 0.20 <= (want[c] == 255).mean() <= 0.42, (c, (want[c] == 255).mean())
    ndiff = [int((want[c] != px[c]).sum()) for c in range(3)]
    print('%d x %d, patch %d at %d, block %d: coverage %s, pixels off the per-pixel masks %s'
          % (h, w, p_size, size, block, [round(float((want[c] == 255).mean()), 3) for c in range(3)], ndiff))
    if p_size == size:
        assert ndiff == [0, 0, 0]
    elif block == 2 and (h, w) == (96, 96):
        assert ndiff == [0, 0, 0]                                            # blocks and 2 x 2 boxes coincide: nothing to resize away
    else:
        assert min(ndiff) >= 200, ndiff                                      # hundreds to thousands of pixels per class
    # the near-miss colours are there, and taking them for their class would change the masks
    assert (lab == COLOURS[4]).all(-1).any() and (lab == COLOURS[5]).all(-1).any() and (lab == COLOURS[3]).all(-1).any()
    if p_size != size and block == 1:                                        # every k of a 2 x 2 box, for every class
        hl = host_labels(A, lab, p_size, p_size, 3)                          # per-pixel selection of every patch
        k = hl[:, :, 0::2, 0::2] + hl[:, :, 0::2, 1::2] + hl[:, :, 1::2, 0::2] + hl[:, :, 1::2, 1::2]
        for c in range(3):
            assert set(np.unique(k[:, c]).astype(int)) == {0, 1, 2, 3, 4}
        assert np.array_equal(host_labels(A, lab, p_size, size, 3), (k >= 2).astype(np.float64))
