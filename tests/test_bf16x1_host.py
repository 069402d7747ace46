"""CPU: the host side of the bf16x1 inference convolution (csrc/conv_halo_k32_bf16.hip) -- exported symbols, host validation before
any launch, the legality predicate on descriptors, the pack size.  No GPU, no launches."""
import ctypes

import pytest

FIVE = ('ssg_conv2d_bf16x1_ok', 'ssg_conv2d_bf16x1_kernel_id', 'ssg_conv2d_bf16x1_f32', 'ssg_pack_weights_bf16x1_bytes', 'ssg_pack_weights_bf16x1')


def _desc(lib, n=1, c1=64, c2=0, cout=64, h=20, w=20, stride=1):
    """Descriptor of a 3x3 pad-1 forward conv over aligned stand-in pointers (the predicate dereferences nothing)."""
    d = lib.ConvDesc()
    d.in1 = 4096; d.C1 = c1; d.ld1 = c1
    if c2:
        d.in2 = 8192; d.C2 = c2; d.ld2 = c2
    d.N, d.H, d.W = n, h, w
    d.w = 12288; d.Kp = 9 * (c1 + c2); d.kmode = 0
    d.out = 16384; d.Cout = cout; d.ldo = cout
    gh, gw = (h - 1) // stride + 1, (w - 1) // stride + 1
    d.GH, d.GW, d.OH, d.OW = gh, gw, gh, gw
    d.in_sy = d.in_sx = stride
    d.out_sy = d.out_sx = 1
    d.ntaps = 9
    for t in range(9):
        d.dy[t] = t // 3 - 1; d.dx[t] = t % 3 - 1
    return d


def test_library_exports_the_five_symbols(pkg):
    lib = ctypes.CDLL(pkg._lib.LIB_PATH)
    for name in FIVE:
        assert hasattr(lib, name), name
        assert name in pkg._lib.SIGNATURES
    assert pkg._lib.load().ssg_abi_version() == 10


def test_launcher_validates_on_the_host(pkg):
    lib = pkg._lib
    d = lib.ConvDesc()
    rc = lib.load().ssg_conv2d_bf16x1_f32(ctypes.byref(d), None, None)
    assert rc != 0 and b'bf16x1' in lib.load().ssg_last_error()
    rc = lib.load().ssg_conv2d_bf16x1_f32(ctypes.byref(_desc(lib)), None, None)        # legal descriptor, no weight pack
    assert rc != 0 and b'bf16x1' in lib.load().ssg_last_error()
    assert lib.call('ssg_conv2d_bf16x1_kernel_id', ctypes.byref(d)) < 0


def test_predicate_on_descriptors(pkg):
    lib = pkg._lib
    ok = lambda d: lib.call('ssg_conv2d_bf16x1_ok', ctypes.byref(d))
    assert ok(_desc(lib)) == 1064 and lib.call('ssg_conv2d_bf16x1_kernel_id', ctypes.byref(_desc(lib))) == 71
    assert ok(_desc(lib, cout=128)) == 1128 and lib.call('ssg_conv2d_bf16x1_kernel_id', ctypes.byref(_desc(lib, cout=128))) == 70
    assert ok(_desc(lib, cout=192, c1=32, c2=64, w=17)) == 1064
    assert ok(_desc(lib, stride=2)) == 0
    assert ok(_desc(lib, c1=48)) == 0
    assert ok(_desc(lib, c1=32, c2=48)) == 0
    assert ok(_desc(lib, w=16)) == 0
    assert ok(_desc(lib, cout=32)) == 0
    # every refused descriptor field, pointers off the 16-byte grid, tensors beyond the 32-bit byte offsets
    for field, value in (('bnpart', 4096), ('ws', 4096), ('parity_merge', 1), ('in_scale', 4096), ('bwd_x', 4096), ('in1', 4100), ('out', 16388),
                         ('ldo', 66), ('kmode', 1), ('act', 3), ('out_oy', 1)):
        d = _desc(lib)
        setattr(d, field, value)
        assert ok(d) == 0, field
    assert ok(_desc(lib, n=64, c1=512, h=256, w=256)) == 0          # 8 GiB of input


def test_pack_is_a_third_of_the_split_pack(pkg):
    lib = pkg._lib
    for r, kp, bn in ((64, 288, 1064), (192, 9 * 96, 1064), (128, 9 * 96, 1128), (512, 9 * 1024, 1128)):
        x1 = lib.call('ssg_pack_weights_bf16x1_bytes', r, kp, bn)
        assert x1 > 0 and 3 * x1 == lib.call('ssg_pack_weights_split_bytes', r, kp, bn)
        assert x1 == r * kp * 2
    assert lib.call('ssg_pack_weights_bf16x1_bytes', 64, 288, 64) == 0
    assert lib.call('ssg_pack_weights_bf16x1_bytes', 96, 288, 1064) == 0
    with pytest.raises(RuntimeError, match='bf16x1'):
        lib.call('ssg_pack_weights_bf16x1', None, 64, 288, 1064, None, None)
