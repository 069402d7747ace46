"""CPU: the host side of the stride-2 bf16x1 kernels (csrc/conv_s2_k32_x1.hip) -- exported symbols, host validation before any
launch, the two legality predicates on descriptors, kernel ids, the tap-count-aware pack size.  No GPU, no launches."""
import ctypes

import pytest

NEW = ('ssg_conv2d_bf16x1_s2_ok', 'ssg_conv2d_bf16x1_s2_kernel_id', 'ssg_conv2d_bf16x1_s2_f32', 'ssg_conv2d_bf16x1_cls_ok',
       'ssg_conv2d_bf16x1_cls_kernel_id', 'ssg_conv2d_bf16x1_cls_f32', 'ssg_pack_weights_bf16x1_taps_bytes', 'ssg_pack_weights_bf16x1_taps')
CLASSES = [(0, 0, [(0, 0)]), (0, 1, [(0, 1), (0, 0)]), (1, 0, [(1, 0), (0, 0)]), (1, 1, [(1, 1), (1, 0), (0, 1), (0, 0)])]


def _fwd(lib, n=1, c1=64, cout=64, h=20, w=40):
    """Descriptor of a 3x3 stride-2 pad-1 forward conv over aligned stand-in pointers (the predicate dereferences nothing)."""
    d = lib.ConvDesc()
    d.in1 = 4096; d.C1 = c1; d.ld1 = c1
    d.N, d.H, d.W = n, h, w
    d.w = 12288; d.Kp = 9 * c1; d.kmode = 0
    d.out = 16384; d.Cout = cout; d.ldo = cout
    gh, gw = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    d.GH, d.GW, d.OH, d.OW = gh, gw, gh, gw
    d.in_sy = d.in_sx = 2
    d.out_sy = d.out_sx = 1
    d.ntaps = 9
    for t in range(9):
        d.dy[t] = t // 3 - 1; d.dx[t] = t % 3 - 1
    return d


def _cls(lib, k=3, n=1, o=64, rows=64, h=20, w=40):
    """Descriptor of parity class k of the input gradient [n, rows, h, w] of that conv (dy has `o` channels)."""
    py, px, taps = CLASSES[k]
    d = lib.ConvDesc()
    oh, ow = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    d.in1 = 4096; d.C1 = o; d.ld1 = o
    d.N, d.H, d.W = n, oh, ow
    d.w = 12288; d.Kp = len(taps) * o; d.kmode = 0
    d.out = 16384; d.Cout = rows; d.ldo = rows
    d.GH, d.GW, d.OH, d.OW = (h - py + 1) // 2, (w - px + 1) // 2, h, w
    d.in_sy = d.in_sx = 1
    d.out_sy = d.out_sx = 2
    d.out_oy, d.out_ox = py, px
    d.ntaps = len(taps)
    for t, (oy, ox) in enumerate(taps):
        d.dy[t] = oy; d.dx[t] = ox
    return d


def test_library_exports_the_new_symbols(pkg):
    lib = ctypes.CDLL(pkg._lib.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in pkg._lib.SIGNATURES
    assert pkg._lib.load().ssg_abi_version() == 10


def test_launchers_validate_on_the_host(pkg):
    lib = pkg._lib
    for entry, tag, legal in (('ssg_conv2d_bf16x1_s2_f32', b'bf16x1 s2', _fwd(lib)), ('ssg_conv2d_bf16x1_cls_f32', b'bf16x1 cls', _cls(lib))):
        fn = getattr(lib.load(), entry)
        assert fn(None, None, None) != 0 and tag in lib.load().ssg_last_error()                 # null descriptor
        assert b'null desc' in lib.load().ssg_last_error()
        assert fn(ctypes.byref(lib.ConvDesc()), None, None) != 0 and tag in lib.load().ssg_last_error()
        assert fn(ctypes.byref(legal), None, None) != 0 and b'weight pack' in lib.load().ssg_last_error()   # legal descriptor, no pack
    assert lib.call('ssg_conv2d_bf16x1_s2_kernel_id', ctypes.byref(lib.ConvDesc())) < 0
    assert lib.call('ssg_conv2d_bf16x1_cls_kernel_id', ctypes.byref(lib.ConvDesc())) < 0
    assert lib.call('ssg_conv2d_bf16x1_s2_ok', None) == 0 and lib.call('ssg_conv2d_bf16x1_cls_ok', None) == 0


def test_forward_predicate_on_descriptors(pkg):
    lib = pkg._lib
    ok = lambda d: lib.call('ssg_conv2d_bf16x1_s2_ok', ctypes.byref(d))
    kid = lambda d: lib.call('ssg_conv2d_bf16x1_s2_kernel_id', ctypes.byref(d))
    assert ok(_fwd(lib)) == 1064 and kid(_fwd(lib)) == 74
    assert ok(_fwd(lib, cout=128)) == 1128 and kid(_fwd(lib, cout=128)) == 73
    # the discriminator's four stride-2 layers at 16 x 512^2, odd sizes, the minimum width
    for c, s in ((64, 512), (128, 256), (256, 128), (512, 64)):
        assert ok(_fwd(lib, n=16, c1=c, cout=c, h=s, w=s)) == (1064 if c == 64 else 1128)
    assert ok(_fwd(lib, c1=32, cout=192, h=19, w=33)) == 1064
    assert ok(_fwd(lib, w=32)) == 0                                  # output 16 wide
    assert ok(_fwd(lib, c1=48)) == 0
    assert ok(_fwd(lib, cout=32)) == 0
    for field, value in (('bnpart', 4096), ('ws', 4096), ('parity_merge', 1), ('in_scale', 4096), ('bwd_x', 4096), ('res', 4096), ('in2', 4096),
                         ('C2', 32), ('in1', 4100), ('out', 16388), ('w', 12292), ('bias', 4100), ('ldo', 66), ('ld1', 66), ('kmode', 1), ('act', 3),
                         ('out_oy', 1), ('out_ox', 1), ('in_sy', 1), ('in_sx', 1), ('out_sy', 2), ('ntaps', 4), ('Kp', 64 * 9 + 16), ('GW', 21), ('GH', 11)):
        d = _fwd(lib)
        setattr(d, field, value)
        assert ok(d) == 0, field
    d = _fwd(lib); d.dy[0], d.dy[1] = d.dy[1], d.dy[0]; d.dx[0], d.dx[1] = d.dx[1], d.dx[0]
    assert ok(d) == 0                                                # not row-major
    assert ok(_fwd(lib, n=64, c1=512, h=256, w=256)) == 0            # 8 GiB of input
    # what the unit-stride predicate keeps refusing is not changed by the new entry points
    assert lib.call('ssg_conv2d_bf16x1_ok', ctypes.byref(_fwd(lib))) == 0


def test_class_predicate_on_descriptors(pkg):
    lib = pkg._lib
    ok = lambda d: lib.call('ssg_conv2d_bf16x1_cls_ok', ctypes.byref(d))
    kid = lambda d: lib.call('ssg_conv2d_bf16x1_cls_kernel_id', ctypes.byref(d))
    assert [kid(_cls(lib, k)) for k in range(4)] == [76, 78, 78, 80]
    assert [kid(_cls(lib, k, rows=128)) for k in range(4)] == [75, 77, 77, 79]
    assert all(ok(_cls(lib, k, n=2, o=32, rows=64, h=21, w=71)) == 1064 for k in range(4))
    assert all(ok(_cls(lib, k, h=18, w=34)) == 1064 for k in range(4))       # every class grid 17 wide
    assert ok(_cls(lib, 0, w=33)) == 1064 and ok(_cls(lib, 1, w=33)) == 0    # class px = 1 is 16 wide
    assert ok(_cls(lib, o=48)) == 0 and ok(_cls(lib, rows=32)) == 0
    for field, value in (('bnpart', 4096), ('ws', 4096), ('parity_merge', 1), ('in_scale', 4096), ('bwd_x', 4096), ('res', 4096), ('in2', 4096),
                         ('in1', 4100), ('out', 16388), ('ldo', 66), ('kmode', 1), ('act', 3), ('out_oy', 2), ('out_ox', -1), ('in_sy', 2),
                         ('out_sy', 1), ('out_sx', 1), ('ntaps', 3), ('ntaps', 9), ('Kp', 64 * 9), ('GH', 11), ('GW', 21)):
        d = _cls(lib)
        setattr(d, field, value)
        assert ok(d) == 0, field
    d = _cls(lib); d.dy[0] = 2
    assert ok(d) == 0                                                # offset outside {0, +1}
    d = _cls(lib); d.dx[1] = -1
    assert ok(d) == 0
    d = _cls(lib); d.dy[1], d.dx[1] = d.dy[0], d.dx[0]
    assert ok(d) == 0                                                # a tap twice
    assert lib.call('ssg_conv2d_bf16x1_ok', ctypes.byref(_cls(lib))) == 0
    assert lib.call('ssg_conv2d_bf16x1_s2_ok', ctypes.byref(_cls(lib))) == 0


def test_tap_count_aware_pack_size(pkg):
    lib = pkg._lib
    for r, o, nt, bn in ((64, 64, 1, 1064), (64, 64, 2, 1064), (192, 96, 4, 1064), (128, 32, 4, 1128), (512, 512, 2, 1128)):
        assert lib.call('ssg_pack_weights_bf16x1_taps_bytes', r, nt * o, nt, bn) == r * nt * o * 2
    # nine taps: the size of the existing pack, whose own contract (Kp % 288 == 0) is unchanged
    assert lib.call('ssg_pack_weights_bf16x1_taps_bytes', 64, 288, 9, 1064) == lib.call('ssg_pack_weights_bf16x1_bytes', 64, 288, 1064)
    assert lib.call('ssg_pack_weights_bf16x1_bytes', 64, 128, 1064) == 0
    assert lib.call('ssg_pack_weights_bf16x1_taps_bytes', 64, 128, 4, 64) == 0          # not a format code
    assert lib.call('ssg_pack_weights_bf16x1_taps_bytes', 96, 128, 4, 1064) == 0        # rows % 64
    assert lib.call('ssg_pack_weights_bf16x1_taps_bytes', 64, 96, 2, 1064) == 0         # Kp % (32 * ntaps)
    assert lib.call('ssg_pack_weights_bf16x1_taps_bytes', 64, 64, 0, 1064) == 0
    with pytest.raises(RuntimeError, match='bf16x1 taps'):
        lib.call('ssg_pack_weights_bf16x1_taps', None, 64, 128, 4, 1064, None, None)
