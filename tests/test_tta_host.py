"""CPU: the host side of test-time augmentation -- `ops.tta_codes`, the checks of `segment_image` / `evaluate_image` that run before
any GPU use, the two exported entry points (`ssg_sw_gather_patches_d4_u8_f32`, `ssg_sw_tta_reduce_f32`) and their argument checks,
which precede any launch.  No GPU, no launches."""
import ctypes
import inspect
import os
import re

import pytest

from conftest import ROOT

TWO = ('ssg_sw_gather_patches_d4_u8_f32', 'ssg_sw_tta_reduce_f32')
CFG = dict(patch_size=64, input_w=32, input_h=32, patch_overlap=0.5, num_classes=3)
BAD = ('bogus', 'D4', '', (0, 1, 2), (0, 0), (0, 4, 4, 2), (0, 8), (-1, 0), (), tuple(range(8)) + (0,), (0.0, 4.0), (True, 0), 4, 0, {0, 4})


def test_tta_codes_accepts(pkg):
    t = pkg.ops.tta_codes
    assert t(None) == (0,)
    assert t('hflip') == (0, 4) and t('flips') == (0, 4, 2, 6) and t('d4') == (0, 1, 2, 3, 4, 5, 6, 7)
    assert t((3,)) == (3,) and t([5, 2]) == (5, 2) and t((7, 0, 1, 6)) == (7, 0, 1, 6)
    assert t((7, 6, 5, 4, 3, 2, 1, 0)) == (7, 6, 5, 4, 3, 2, 1, 0)          # list order is kept: it is the order of the tree


@pytest.mark.parametrize('bad', BAD, ids=repr)
def test_tta_codes_rejects(pkg, bad):
    with pytest.raises(ValueError, match='tta'):
        pkg.ops.tta_codes(bad)


@pytest.mark.parametrize('bad', ['bogus', (0, 1, 2), (0, 0), (0, 8)], ids=repr)
def test_api_raises_before_any_gpu_use(pkg, bad):
    A = pkg.aerial_image_segmentation_api
    with pytest.raises(ValueError, match='tta'):
        A.segment_image(None, None, CFG, tta=bad)
    with pytest.raises(ValueError, match='tta'):
        A.evaluate_image(None, None, None, CFG, tta=bad)
    with pytest.raises(ValueError, match='tta'):
        A.evaluate_images(None, [(None, None)], CFG, tta=bad)
    with pytest.raises(ValueError, match='tta'):
        A._device_masks(None, None, CFG, 12, True, 'fp32', None, 'segment_image', bad)


def test_signatures(pkg):
    A, ops = pkg.aerial_image_segmentation_api, pkg.ops
    for fn in (A._device_masks, A.segment_image, A.evaluate_image, A.evaluate_images):
        assert inspect.signature(fn).parameters['tta'].default is None
    assert inspect.signature(ops.sw_gather_patches).parameters['orient'].default == 0
    assert list(inspect.signature(ops.sw_tta_reduce).parameters) == ['stack', 'codes', 'out']


def test_wrappers_check_before_any_launch(pkg):
    import torch
    ops = pkg.ops
    img = torch.zeros(96, 96, 3, dtype=torch.uint8)
    for bad in (8, -1, 1.0, True, None):
        with pytest.raises(ValueError, match='orient'):
            ops.sw_gather_patches(img, [(0, 0)], 64, 32, orient=bad)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.sw_gather_patches(img, [(0, 0)], 64, 32, orient=3)
    stack = torch.zeros(2, 1, 3, 8, 8)
    with pytest.raises(ValueError, match='tta'):
        ops.sw_tta_reduce(stack, (0, 0))
    with pytest.raises(ValueError, match='3 views'):
        ops.sw_tta_reduce(stack, (0, 1, 2))
    with pytest.raises(ValueError, match='2 views for 4 codes'):
        ops.sw_tta_reduce(stack, 'flips')
    with pytest.raises(ValueError, match='K, B, C, S, S'):
        ops.sw_tta_reduce(stack[0], (0,))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.sw_tta_reduce(stack, 'hflip')


def test_symbols_in_library_header_and_ctypes_table(pkg):
    lib = ctypes.CDLL(pkg._lib.LIB_PATH)
    header = open(os.path.join(ROOT, 'include', 'ssunet_hip.h')).read()
    for name in TWO:
        assert hasattr(lib, name), name
        assert name in pkg._lib.SIGNATURES, name
        assert re.search(r'\b%s\s*\(' % name, header), name
    assert pkg._lib.load().ssg_abi_version() == 10 == pkg._lib.ABI_VERSION    # additive: new symbols only


def test_entries_refuse_bad_arguments_without_a_launch(pkg):
    lib = pkg._lib
    L = lib.load()
    fake = ctypes.c_void_p(4096)                                             # stands for device memory: never dereferenced
    org = (ctypes.c_int32 * 2)(0, 0)
    norm = (1.0, 1.0, 1.0, 1.0, 1.0, 1.0)

    def refused(rc, *words):
        msg = L.ssg_last_error()
        assert rc != 0 and all(w in msg for w in words), (rc, msg)

    gather = L.ssg_sw_gather_patches_d4_u8_f32
    for orient in (8, -1, 100):
        refused(gather(fake, 96, 96, fake, org, 1, 64, 32, orient, *norm, fake, None), b'sw_gather_d4', b'orient %d' % orient)
    refused(gather(None, 96, 96, fake, org, 1, 64, 32, 1, *norm, fake, None), b'sw_gather_d4', b'null')
    refused(gather(fake, 96, 96, fake, None, 1, 64, 32, 1, *norm, fake, None), b'sw_gather_d4', b'null')
    refused(gather(fake, 96, 96, fake, org, 1, 48, 16, 1, *norm, fake, None), b'sw_gather_d4', b'factors 1 and 2')
    refused(gather(fake, 96, 96, fake, org, 0, 64, 32, 1, *norm, fake, None), b'sw_gather_d4', b'P 0')
    out_org = (ctypes.c_int32 * 2)(33, 0)
    refused(gather(fake, 96, 96, fake, out_org, 1, 64, 32, 5, *norm, fake, None), b'sw_gather_d4', b'outside')
    refused(gather(fake, 96, 96, fake, org, 1, 64, 32, 5, *norm, ctypes.c_void_p(4100), None), b'sw_gather_d4', b'aligned')

    reduce = L.ssg_sw_tta_reduce_f32

    def codes(*c):
        return (ctypes.c_int32 * max(len(c), 1))(*c)

    slab = 3 * 8 * 8 * 4
    for k in (0, 3, 5, 6, 7, 9, 16, -1):
        refused(reduce(fake, slab, 4, k, codes(*range(8)), 3, 3, 8, fake, 4, None), b'sw_tta_reduce', b'%d views' % k)
    refused(reduce(fake, slab, 4, 2, codes(0, 8), 3, 3, 8, fake, 4, None), b'sw_tta_reduce', b'code 8')
    refused(reduce(fake, slab, 4, 2, codes(-1, 0), 3, 3, 8, fake, 4, None), b'sw_tta_reduce', b'code -1')
    refused(reduce(fake, slab, 4, 4, codes(0, 4, 2, 4), 3, 3, 8, fake, 4, None), b'sw_tta_reduce', b'code 4 is repeated')
    refused(reduce(fake, slab, 4, 8, codes(0, 1, 2, 3, 4, 5, 6, 0), 3, 3, 8, fake, 4, None), b'sw_tta_reduce', b'repeated')
    refused(reduce(fake, slab, 4, 2, codes(0, 4), 3, 5, 8, fake, 8, None), b'sw_tta_reduce', b'5 channels')      # C > ld
    refused(reduce(fake, 3 * 8 * 8 * 8, 8, 2, codes(0, 4), 3, 5, 8, fake, 4, None), b'sw_tta_reduce', b'5 channels')   # C > ldo
    refused(reduce(fake, slab, 4, 2, codes(0, 4), 3, 3, 0, fake, 4, None), b'sw_tta_reduce', b'S 0')
    refused(reduce(fake, slab, 4, 2, codes(0, 4), 3, 3, -8, fake, 4, None), b'sw_tta_reduce', b'S -8')
    refused(reduce(fake, slab, 4, 2, codes(0, 4), 0, 3, 8, fake, 4, None), b'sw_tta_reduce', b'B 0')
    refused(reduce(fake, slab, 4, 2, codes(0, 4), 3, 0, 8, fake, 4, None), b'sw_tta_reduce', b'C 0')
    refused(reduce(None, slab, 4, 2, codes(0, 4), 3, 3, 8, fake, 4, None), b'sw_tta_reduce', b'null')
    refused(reduce(fake, slab, 4, 2, None, 3, 3, 8, fake, 4, None), b'sw_tta_reduce', b'null')
    refused(reduce(fake, slab, 4, 2, codes(0, 4), 3, 3, 8, None, 4, None), b'sw_tta_reduce', b'null')
    refused(reduce(fake, slab - 4, 4, 2, codes(0, 4), 3, 3, 8, fake, 4, None), b'sw_tta_reduce', b'view stride')
    refused(reduce(fake, slab, 4, 2, codes(0, 4), 3, 3, 8, ctypes.c_void_p(4100), 4, None), b'sw_tta_reduce', b'aligned')
    refused(reduce(fake, slab, 6, 2, codes(0, 4), 3, 3, 8, fake, 4, None), b'sw_tta_reduce', b'multiples of 4')
    with pytest.raises(RuntimeError, match='ssg_sw_gather_patches_d4_u8_f32 failed'):
        lib.call('ssg_sw_gather_patches_d4_u8_f32', fake, 96, 96, fake, org, 1, 64, 32, 8, *norm, fake, None)
    with pytest.raises(RuntimeError, match='ssg_sw_tta_reduce_f32 failed'):
        lib.call('ssg_sw_tta_reduce_f32', fake, slab, 4, 3, codes(0, 1, 2), 3, 3, 8, fake, 4, None)
