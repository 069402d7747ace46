"""CPU: the host side of precision 'bf16x2' -- the nine exported symbols, host validation before any launch, the predicates on
descriptors, the pack size, the precision strings and their illegal combinations, the config plumbing.  No GPU, no launches."""
import ctypes
import os
import re

import pytest

from conftest import ROOT
from test_bf16x1_host import _desc

NINE = ('ssg_conv2d_bf16x2_ok', 'ssg_conv2d_bf16x2_kernel_id', 'ssg_conv2d_bf16x2_f32', 'ssg_pack_weights_bf16x2_bytes',
        'ssg_pack_weights_bf16x2', 'ssg_conv2d_wgrad_bf16x2_ok', 'ssg_conv2d_wgrad_bf16x2_workspace_bytes', 'ssg_conv2d_wgrad_bf16x2_f32',
        'ssg_conv2d_wgrad_bf16x2_kernel_id')


def _wdesc(lib, n=1, c1=64, c2=0, cout=64, h=20, w=20, stride=1):
    d = lib.WgradDesc()
    d.in1 = 4096; d.C1 = c1; d.ld1 = c1
    if c2:
        d.in2 = 8192; d.C2 = c2; d.ld2 = c2
    d.N, d.H, d.W = n, h, w
    d.dout = 12288; d.ldd = cout; d.Cout = cout
    d.GH, d.GW = (h - 1) // stride + 1, (w - 1) // stride + 1
    d.in_sy = d.in_sx = stride
    d.ntaps = 9
    for t in range(9):
        d.dy[t] = t // 3 - 1; d.dx[t] = t % 3 - 1; d.ky[t] = t // 3; d.kx[t] = t % 3
    d.KH = d.KW = 3; d.Cin_real = c1 + c2
    return d


def test_symbols_in_library_header_and_ctypes_table(pkg):
    lib = ctypes.CDLL(pkg._lib.LIB_PATH)
    header = open(os.path.join(ROOT, 'include', 'ssunet_hip.h')).read()
    for name in NINE:
        assert hasattr(lib, name), name
        assert name in pkg._lib.SIGNATURES, name
        assert re.search(r'\b%s\s*\(' % name, header), name
    for kid in ('90 / 91', '92 ='):
        assert kid in header


def test_kernel_ids_are_new(pkg):
    ops = pkg.ops
    new = set(ops._X2_LABELS) | set(ops._WGRAD_X2_LABELS)
    assert new == {90, 91, 92}
    old = (set(ops._CONV_LABELS) | set(ops._WGRAD_LABELS) | set(ops._X1_LABELS) | set(ops._WGRAD_X1_LABELS) | set(ops._X1_S2_LABELS)
           | set(ops._X1_CLS_LABELS) | set(ops._WGRAD_X1_S2_LABELS))
    assert not new & old


def test_launchers_validate_on_the_host(pkg):
    lib = pkg._lib
    d = lib.ConvDesc()
    assert lib.load().ssg_conv2d_bf16x2_f32(ctypes.byref(d), None, None) != 0 and b'bf16x2' in lib.load().ssg_last_error()
    assert lib.load().ssg_conv2d_bf16x2_f32(ctypes.byref(_desc(lib)), None, None) != 0        # legal descriptor, no weight pack
    assert b'bf16x2' in lib.load().ssg_last_error()
    assert lib.call('ssg_conv2d_bf16x2_kernel_id', ctypes.byref(d)) < 0
    wd = lib.WgradDesc()
    assert lib.load().ssg_conv2d_wgrad_bf16x2_f32(ctypes.byref(wd), None) != 0 and b'bf16x2' in lib.load().ssg_last_error()
    assert lib.call('ssg_conv2d_wgrad_bf16x2_kernel_id', ctypes.byref(wd)) < 0
    assert lib.call('ssg_conv2d_wgrad_bf16x2_workspace_bytes', ctypes.byref(wd)) == 0


def test_conv_predicate_on_descriptors(pkg):
    lib = pkg._lib
    ok = lambda d: lib.call('ssg_conv2d_bf16x2_ok', ctypes.byref(d))
    kid = lambda d: lib.call('ssg_conv2d_bf16x2_kernel_id', ctypes.byref(d))
    assert ok(_desc(lib)) == 2064 and kid(_desc(lib)) == 91
    assert ok(_desc(lib, cout=128)) == 2128 and kid(_desc(lib, cout=128)) == 90
    assert ok(_desc(lib, cout=192, c1=32, c2=64, w=17)) == 2064
    for kw in (dict(stride=2), dict(c1=48), dict(c1=32, c2=48), dict(w=16), dict(cout=32), dict(cout=96)):
        assert ok(_desc(lib, **kw)) == 0 and kid(_desc(lib, **kw)) < 0, kw
    for field, value in (('bnpart', 4096), ('ws', 4096), ('parity_merge', 1), ('in_scale', 4096), ('bwd_x', 4096), ('in1', 4100), ('out', 16388),
                         ('ldo', 66), ('kmode', 1), ('act', 3), ('out_oy', 1)):
        d = _desc(lib)
        setattr(d, field, value)
        assert ok(d) == 0, field
    d = _desc(lib)
    d.dx[4] = 2                                                         # a wrong tap set
    assert ok(d) == 0
    assert ok(_desc(lib, n=64, c1=512, h=256, w=256)) == 0             # 8 GiB of input
    # the one-term entry points answer as before
    assert lib.call('ssg_conv2d_bf16x1_ok', ctypes.byref(_desc(lib))) == 1064


def test_wgrad_predicate_on_descriptors(pkg):
    lib = pkg._lib
    ok = lambda d: lib.call('ssg_conv2d_wgrad_bf16x2_ok', ctypes.byref(d))
    d = _wdesc(lib)
    assert ok(d) == 1 and lib.call('ssg_conv2d_wgrad_bf16x2_kernel_id', ctypes.byref(d)) == 92
    assert lib.call('ssg_conv2d_wgrad_bf16x2_workspace_bytes', ctypes.byref(d)) == lib.call('ssg_conv2d_wgrad_bf16x1_workspace_bytes', ctypes.byref(d)) > 0
    assert ok(_wdesc(lib, c1=64, c2=64, cout=192, w=17)) == 1
    for kw in (dict(stride=2), dict(c1=32), dict(w=16), dict(cout=96), dict(c1=64, c2=32)):
        assert ok(_wdesc(lib, **kw)) == 0, kw
    d = _wdesc(lib)
    d.dx[4] = 1
    assert ok(d) == 0
    d = _wdesc(lib)
    d.in_scale = 4096
    assert ok(d) == 0


def test_pack_is_twice_the_one_term_pack(pkg):
    lib = pkg._lib
    for r, kp, bn in ((64, 288, 64), (192, 9 * 96, 64), (128, 9 * 96, 128), (512, 9 * 1024, 128)):
        x2 = lib.call('ssg_pack_weights_bf16x2_bytes', r, kp, 2000 + bn)
        assert x2 == r * kp * 4 == 2 * lib.call('ssg_pack_weights_bf16x1_bytes', r, kp, 1000 + bn)
    assert lib.call('ssg_pack_weights_bf16x2_bytes', 64, 288, 1064) == 0
    assert lib.call('ssg_pack_weights_bf16x2_bytes', 96, 288, 2064) == 0
    with pytest.raises(RuntimeError, match='bf16x2'):
        lib.call('ssg_pack_weights_bf16x2', None, 64, 288, 2064, None, None)


def test_precision_strings(pkg):
    ops = pkg.ops
    assert ops._PRECISIONS == ('fp32', 'bf16x1', 'bf16x2')
    for ctx, mode in ((ops.infer_precision, ops.infer_precision_mode), (ops.train_precision, ops.train_precision_mode)):
        with ctx('bf16x2'):
            assert mode() == 'bf16x2'
            with ctx('bf16x1'):
                assert mode() == 'bf16x1'
            assert mode() == 'bf16x2'
        assert mode() == 'fp32'
        for bad in ('bf16', 'medium', 'x1', 'fp16', 'x2', 'bf16x3'):
            with pytest.raises(ValueError):
                ctx(bad)


def test_illegal_combinations(pkg):
    ops = pkg.ops
    with pytest.raises(ValueError, match='wgrad_s2'):
        ops.train_precision('bf16x2', wgrad_s2='bf16x1')
    with pytest.raises(ValueError, match='wgrad_s2'):
        ops.train_precision('bf16x2', wgrad_s2='bf16x2')
    with pytest.raises(ValueError, match='wgrad_s2'):
        ops._check_wgrad_s2('conv2d', 'bf16x2', 'bf16x1')
    ops._check_wgrad_s2('conv2d', 'bf16x2', 'fp32')
    ops._check_wgrad_s2('conv2d', 'bf16x1', 'bf16x1')
    # the routing predicate: unit stride and pad 1 only; fused transforms are refused as under 'bf16x1'
    assert ops._x1_routed('bf16x2', 1, 1, None, None) and not ops._x1_routed('bf16x2', 2, 1, None, None)
    assert not ops._x1_routed('bf16x2', 1, 0, None, None) and not ops._x1_routed('fp32', 1, 1, None, None)
    assert not ops._x1_s2_routed('bf16x2', True, 2, 1, None)                 # stride 2 stays fp32-class
    for fused in ((1, 2, 3, 4),):
        with pytest.raises(ValueError, match='in_affine / bwd_stats'):
            ops._x1_routed('bf16x2', 1, 1, None, fused)
        with pytest.raises(ValueError, match='in_affine / bwd_stats'):
            ops._x1_routed('bf16x1', 1, 1, None, fused)
    with pytest.raises(ValueError):
        ops._x1_routed('medium', 1, 1, None, None)


def test_gan_step_and_config_plumbing(pkg):
    """d_precision keeps its two values (checked before anything runs); both trainers hand config['precision'] to train_precision,
    which takes 'bf16x2'."""
    import inspect
    T = pkg.train_seg_gan
    with pytest.raises(ValueError, match='d_precision'):
        T.gan_step(None, None, None, None, None, None, None, None, None, 3, d_precision='bf16x2')
    with pytest.raises(ValueError, match='d_precision'):
        T.gan_step(None, None, None, None, None, None, None, None, None, 3, d_precision='medium')
    with pytest.raises(ValueError, match='wgrad_s2'):
        T.gan_step(None, None, None, None, None, None, None, None, None, 3, precision='bf16x2', d_wgrad_s2='bf16x1')
    assert "config.get('precision', 'fp32')" in inspect.getsource(T.train)
    assert "config.get('precision', 'fp32')" in inspect.getsource(pkg.train)
    A = pkg.aerial_image_segmentation_api
    for fn in (A.infer_patches, A.segment_image, A.segmentation_inference_full):
        assert 'precision' in inspect.signature(fn).parameters
