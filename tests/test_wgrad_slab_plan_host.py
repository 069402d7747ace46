"""CPU: the slab plan of the weight-gradient kernels whose K-step is one image row of a 32-pixel column strip (ssg_wgrad_slabs in
csrc/conv_wgrad_args.h: wgrad_k32 behind ssg_conv2d_wgrad_f32 with flags = 1, and the bf16x1 / bf16x2 / bf16x1-s2 launchers), restated
here and compared through the *_workspace_bytes queries over a sweep of descriptors.  No GPU, no launches."""
import ctypes

import pytest

NS = (1, 2, 16)
SIZES = (17, 19, 33, 40, 64, 100, 127, 256, 512)             # square H = W
CHANNELS = (64, 128, 192, 512)
# rows the square sizes cannot give: fewer than 8 K-steps (hi < lo under the bf16 launchers' 8 .. 128), and a C1 + C2 input
EXTRA = ((1, 5, 20, 64, 0, 64), (1, 3, 40, 128, 0, 128), (1, 9, 40, 64, 0, 128), (2, 40, 40, 64, 128, 128), (16, 127, 127, 128, 64, 192))


def _cdiv(a, b):
    return -(-a // b)


def slabs(steps, tiles, min_rows, max_rows, seen=None):
    """ssg_wgrad_slabs: (splits, steps_per_split).  `seen` collects which way the scan ended."""
    lo = _cdiv(steps, max_rows)
    hi = max(lo, steps // min_rows)
    best, beff, how = lo, 0.0, 'hi < lo' if steps // min_rows < lo else 'ran to the end'
    for sp in range(lo, min(hi, lo + 1024) + 1):
        wg = sp * tiles
        eff = wg / (256.0 * ((wg + 255) // 256))
        if eff > beff + 1e-9:
            beff, best = eff, sp
        if eff >= 0.97 and wg >= 256:
            how = 'early exit'
            break
    if seen is not None:
        seen.add(how)
    sps = _cdiv(steps, best)
    return _cdiv(steps, sps), sps


def fp32_class_max_rows(n, gh, gw, cin, cout):
    """make_plan's WG_K32 branch: at most 128 rows, and never a longer chain than the 16-pixel-step kernels' planner would use on
    this shape (~1024 workgroups, >= 16 steps per slab, <= 512 slabs), and at least 8."""
    steps16 = n * gh * _cdiv(gw, 16)
    mtf, ntf = (cin // 32, _cdiv(cout, 128)) if cout > 64 else (cin // 64, _cdiv(cout, 64))
    wantf = max(1, 1024 // (mtf * ntf))
    if wantf > steps16 // 16:
        wantf = max(steps16 // 16, 1)
    wantf = min(wantf, 512)
    chain_px = _cdiv(steps16, wantf) * 16
    return max(8, min(128, chain_px // 32))


def _desc(lib, n, h, w, c1, c2, cout, stride=1, flags=0):
    d = lib.WgradDesc()
    d.in1 = 4096; d.C1 = c1; d.ld1 = c1
    if c2:
        d.in2 = 8192; d.C2 = c2; d.ld2 = c2
    d.N, d.H, d.W = n, h, w
    d.dout = 12288; d.ldd = cout; d.Cout = cout
    d.GH, d.GW = (h + stride - 1) // stride, (w + stride - 1) // stride
    d.in_sy = d.in_sx = stride
    d.ntaps = 9
    for t in range(9):
        d.dy[t] = t // 3 - 1; d.dx[t] = t % 3 - 1; d.ky[t] = t // 3; d.kx[t] = t % 3
    d.KH = d.KW = 3; d.Cin_real = c1 + c2
    d.flags = flags
    return d


def _shapes():
    for n in NS:
        for s in SIZES:
            for cin in CHANNELS:
                for cout in CHANNELS:
                    yield n, s, s, cin, 0, cout
    yield from EXTRA


def _fits32(n, h, w, gh, gw, cin_ld, cout):
    return n * h * w * cin_ld * 4 <= 0xfffffff0 and n * gh * gw * cout * 4 <= 0xfffffff0


@pytest.fixture(scope='module')
def lib(pkg):
    return pkg._lib


def test_bf16_launchers_follow_the_slab_rule(lib):
    seen, refused = set(), 0
    for stride, entries in ((1, ('ssg_conv2d_wgrad_bf16x1_workspace_bytes', 'ssg_conv2d_wgrad_bf16x2_workspace_bytes')),
                            (2, ('ssg_conv2d_wgrad_bf16x1_s2_workspace_bytes',))):
        for n, h, w, c1, c2, cout in _shapes():
            d = _desc(lib, n, h, w, c1, c2, cout, stride)
            gh, gw, cin = d.GH, d.GW, c1 + c2
            got = [lib.call(e, ctypes.byref(d)) for e in entries]
            assert len(set(got)) == 1, (stride, n, h, w, c1, c2, cout)              # one term and two terms: one plan
            legal = gw >= 17 and _fits32(n, h, w, gh, gw, max(c1, c2), cout) and not (stride == 2 and c2)
            if not legal:
                refused += 1
                assert got[0] == 0, (stride, n, h, w, c1, c2, cout)
                continue
            nj = 4 if cout % 128 == 0 else 2
            tiles = (cin // 64) * (cout // (32 * nj))
            splits, _ = slabs(n * _cdiv(gw, 32) * gh, tiles, 8, 128, seen)
            assert got[0] == splits * 9 * cin * cout * 4, (stride, n, h, w, c1, c2, cout)
    # the sweep reaches every way the scan can end.  Its cap of 1025 counts cannot bind: 256 consecutive counts hold a multiple of 256,
    # a whole number of full waves, which ends the scan -- the model keeps the cap as the library does.
    assert seen == {'hi < lo', 'early exit', 'ran to the end'} and refused > 0


def test_fp32_class_k32_route_follows_the_slab_rule(lib):
    seen, lowered, full = set(), 0, 0
    for n, h, w, c1, c2, cout in _shapes():
        if not _fits32(n, h, w, h, w, max(c1, c2), cout):
            continue                                             # beyond 32-bit byte offsets the descriptor leaves the k32 route
        d = _desc(lib, n, h, w, c1, c2, cout, 1, flags=1)
        assert lib.call('ssg_conv2d_wgrad_kernel_id', ctypes.byref(d)) == 60
        cin = c1 + c2
        max_rows = fp32_class_max_rows(n, h, w, cin, cout)
        lowered += max_rows < 128
        full += max_rows == 128
        splits, _ = slabs(n * _cdiv(w, 32) * h, (cin // 64) * (cout // 64), 8, max_rows, seen)
        assert lib.call('ssg_conv2d_wgrad_workspace_bytes', ctypes.byref(d)) == splits * 9 * cin * cout * 4, (n, h, w, c1, c2, cout, max_rows)
    assert lowered > 0 and full > 0                              # the 16-pixel-chain bound lowers max_rows on some shapes, not on others
    assert seen == {'hi < lo', 'early exit', 'ran to the end'}
