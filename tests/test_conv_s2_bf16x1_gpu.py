"""csrc/conv_s2_k32_x1.hip: the one-term bf16 3x3 stride-2 pad-1 forward conv (ops._conv_s2_bf16x1_impl) and its input gradient
as four parity-class launches (ops._conv_dgrad_s2_bf16x1_impl).  Gates, per case of tests/s2_bf16x1_ref.py (rehearsed on the CPU
in tests/test_s2_bf16x1_ref.py):
  (a) route     the launches are labelled with the new kernel's instantiations, and nothing else; over the file every
                instantiation has run;
  (b) accuracy  against the fp64 result on the bf16-rounded operands: max and rms error <= 2 x those of the fp32-MFMA kernel
                (ops._conv_fwd_impl / _conv_dgrad_impl at stride 2 with ops.MFMA_SPLIT off) on the SAME rounded operands;
  (c) bound     |y - fp64 on the operands as given| <= (2^-8 + 2^-18) conv(|x|, |w|) + 2 x that kernel's max error, elementwise."""
import ctypes

import numpy as np
import pytest
import torch

import bf16x2_ref as X2
import s2_bf16x1_ref as R
import layout_probe as LP

pytestmark = pytest.mark.gpu

# (case, bias?, act name, ops act code, slope)
FWD_VARIANTS = [
    ('one_chunk_odd_partial', False, None, 0, 0.0),
    ('ring_wrap_min_width', False, None, 0, 0.0),
    ('three_column_tiles', False, None, 0, 0.0),
    ('epilogue', True, 'lrelu', 2, 0.2),
    ('epilogue', True, None, 0, 0.0),
    ('long_reduction', False, None, 0, 0.0),
]
_DONE = {}


def _fp32_mfma(ops, fn):
    old = ops.MFMA_SPLIT
    ops.MFMA_SPLIT = False
    try:
        return fn()
    finally:
        ops.MFMA_SPLIT = old


def _profiled(ops, fn):
    ops.PROFILE = []
    try:
        y = fn()
        return y, [p[0] for p in ops.PROFILE]
    finally:
        ops.PROFILE = None


def _run_fwd(pkg, dev, variant):
    if variant in _DONE:
        return _DONE[variant]
    name, epi, act, code, slope = variant
    ops = pkg.ops
    n, ci, co, h, w = R.FWD_CASES[name]
    xc, wc = R.make_fwd_case(name)
    bias = torch.randn(co, generator=torch.Generator().manual_seed(77)) if epi else None
    bd = bias.to(dev) if epi else None
    xd, wd = ops.to_nhwc(xc.to(dev)), wc.to(dev)
    assert ops.conv2d_bf16x1_s2_ok(xd, wd)
    with torch.no_grad():
        y, labels = _profiled(ops, lambda: ops._conv_s2_bf16x1_impl(xd, wd, bd, code, slope))
        y32 = _fp32_mfma(ops, lambda: ops._conv_fwd_impl(ops.to_nhwc(R.rb(xc).to(dev)), None, R.rb(wc).to(dev), bd, 2, 1, code, slope))
    out = dict(y=y.cpu().double(), y32=y32.cpu().double(), labels=labels, ref=R.conv_ref(xc, wc, bias, act, slope),
               exact=R.conv64(xc, wc, bias, act, slope), bound=R.conv_bound(xc, wc))
    _DONE[variant] = out
    return out


def _run_dgrad(pkg, dev, name):
    key = ('dgrad', name)
    if key in _DONE:
        return _DONE[key]
    ops = pkg.ops
    n, o, i, c_lo, c_hi, h, w = R.DGRAD_CASES[name]
    dyc, wc = R.make_dgrad_case(name)
    dyd, wd = ops.to_nhwc(dyc.to(dev)), wc.to(dev)
    with torch.no_grad():
        dx, labels = _profiled(ops, lambda: ops._conv_dgrad_s2_bf16x1_impl(dyd, wd, h, w, c_lo, c_hi))
        assert dx is not None
        dx32 = _fp32_mfma(ops, lambda: ops._conv_dgrad_impl(ops.to_nhwc(R.rb(dyc).to(dev)), R.rb(wc).to(dev), 2, 1, h, w, c_lo, c_hi))
    out = dict(y=dx.cpu().double(), y32=dx32.cpu().double(), labels=labels, ref=R.dgrad_ref(dyc, wc, h, w, c_lo, c_hi),
               exact=R.dgrad64(dyc, wc, h, w, c_lo, c_hi), bound=R.dgrad_bound(dyc, wc, h, w, c_lo, c_hi))
    _DONE[key] = out
    return out


def _check_gates(tag, r):
    b_ok, c_ok, (em, er, bm, br) = R.gates(r['y'], r['y32'], r['ref'], r['exact'], r['bound'])
    print('%s: x1 max %.3e rms %.3e | fp32 MFMA on the rounded operands max %.3e rms %.3e | worst error / a-priori bound %.3f'
          % (tag, em, er, bm, br, ((r['y'] - r['exact']).abs() / r['bound'].clamp_min(1e-300)).max().item()))
    assert b_ok, (em, er, bm, br)                                                        # (b)
    assert c_ok                                                                          # (c)


@pytest.mark.parametrize('variant', FWD_VARIANTS, ids=lambda v: '%s-%s%s' % (v[0], v[2], '-bias' if v[1] else ''))
def test_forward_route_accuracy_and_bound(pkg, dev, variant):
    r = _run_fwd(pkg, dev, variant)
    co = R.FWD_CASES[variant[0]][2]
    assert r['labels'] == ['conv_s2_k32_x1_kernel<%d,9>' % (128 if co % 128 == 0 else 64)], r['labels']      # (a)
    _check_gates(variant[0], r)


@pytest.mark.parametrize('name', sorted(R.DGRAD_CASES))
def test_input_gradient_route_accuracy_and_bound(pkg, dev, name):
    r = _run_dgrad(pkg, dev, name)
    _, _, _, c_lo, c_hi, _, _ = R.DGRAD_CASES[name]
    bn = 128 if (c_hi - c_lo) % 128 == 0 else 64
    assert r['labels'] == ['conv_s2_k32_x1_kernel<%d,%d>' % (bn, t) for t in (1, 2, 2, 4)], r['labels']       # (a)
    _check_gates(name, r)


def test_every_new_instantiation_ran(pkg, dev):
    seen = set()
    for v in FWD_VARIANTS:
        seen |= set(_run_fwd(pkg, dev, v)['labels'])
    assert seen == set(pkg.ops._X1_S2_LABELS.values()), seen
    seen = set()
    for name in R.DGRAD_CASES:
        seen |= set(_run_dgrad(pkg, dev, name)['labels'])
    assert seen == set(pkg.ops._X1_CLS_LABELS.values()), seen


def _bf16_bits(t):
    """bf16 (round to nearest even, R.rb) bit patterns of an fp32 tensor, as a numpy uint16 array."""
    return (R.rb(t).numpy().view(np.uint32) >> 16).astype(np.uint16)


def _pack_x1_taps_ref(wp, ntaps, bn):
    """ssg_pack_weights_bf16x1_taps restated (bf16x2_ref.pack_x2 with one plane and any tap count).  wp: fp32 [R, Kp] in kmode 0 with
    `ntaps` taps (k = (chunk16 * ntaps + tap) * 16 + c) -> uint16 [R / bn][Kp / 32 steps = chunk32 * ntaps + tap][bn / 16 fragments]
    [64 lanes][8 values]: lane l of fragment j holds row j * 16 + (l & 15), channels chunk32 * 32 + (l >> 4) * 8 .. + 7."""
    rows, kp = wp.shape
    bits = _bf16_bits(wp)
    out = np.zeros((rows // bn, kp // 32, bn // 16, 64, 8), dtype=np.uint16)
    for s in range(kp // 32):
        chunk32, tap = divmod(s, ntaps)
        for g in range(4):
            k0 = ((chunk32 * 2 + (g >> 1)) * ntaps + tap) * 16 + (g & 1) * 8
            out[:, s, :, 16 * g:16 * g + 16, :] = bits[:, k0:k0 + 8].reshape(rows // bn, bn // 16, 16, 8)
    return out


@pytest.mark.parametrize('rows,cin', [(64, 32), (64, 64), (128, 32), (128, 64)])
def test_pack_bytes_match_the_restatement_for_every_tap_count(pkg, dev, rows, cin):
    """The one pack kernel behind ssg_pack_weights_bf16x1 / _bf16x1_taps / _bf16x2, bitwise: both column tiles, one and two 32-channel
    chunks, every tap count, values whose bf16 rounding is a tie (to even: down and up, both signs)."""
    ops, lib = pkg.ops, pkg._lib
    bn = 128 if rows % 128 == 0 else 64

    def packed(entry, wp, fmt, nbytes, *taps):
        assert lib.call(entry + '_bytes', rows, wp.shape[1], *taps, fmt) == nbytes
        buf = torch.zeros(nbytes // 2, dtype=torch.int16, device=dev)
        wd = wp.to(dev)
        lib.call(entry, wd.data_ptr(), rows, wp.shape[1], *taps, fmt, ops.ptr(buf), ops.stream_ptr())
        return buf.cpu().numpy().view(np.uint16)

    g = torch.Generator().manual_seed(77 + rows + cin)
    for ntaps in (1, 2, 4, 9):
        kp = cin * ntaps
        wp = torch.randn(rows, kp, generator=g)
        ties = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8), 2.0 ** -20 * (1 + 5 * 2.0 ** -8)])
        wp.view(-1)[torch.randperm(rows * kp, generator=g)[:4 * len(ties)]] = ties.repeat(4)
        assert ((wp.view(torch.int32) & 0xffff) == 0x8000).sum() >= 4 * len(ties)   # halfway between two bf16 values
        want = _pack_x1_taps_ref(wp, ntaps, bn)
        got = packed('ssg_pack_weights_bf16x1_taps', wp, 1000 + bn, rows * kp * 2, ntaps)
        assert np.array_equal(got.reshape(want.shape), want), ntaps
        if ntaps == 9:
            assert np.array_equal(packed('ssg_pack_weights_bf16x1', wp, 1000 + bn, rows * kp * 2), got)
            want2 = X2.pack_x2(wp.numpy(), bn)
            assert np.array_equal(want2[:, :, 0], want)                              # plane 0 of two terms is the one-term pack
            got2 = packed('ssg_pack_weights_bf16x2', wp, 2000 + bn, rows * kp * 4)
            assert np.array_equal(got2.reshape(want2.shape), want2)


def test_channel_slices_of_wider_tensors(pkg, dev):
    """x / dy and the destinations are channel slices (ld > C) of canary-filled, guarded buffers: same bits as on dense tensors,
    neighbouring lanes and guard bands untouched, every element of the destination written -- for the gradient, by exactly one of
    the four strided class launches (a second write would show as different bits against the dense run only by luck, so each
    class is also run ALONE into a fresh canary buffer and must write its own parity positions and nothing else)."""
    ops = pkg.ops
    g = torch.Generator().manual_seed(5)
    n, c, co, h, w = 1, 64, 64, 11, 38
    xc = torch.randn(n, c, h, w, generator=g) * 1.5 + 0.3
    wc = (torch.randn(co, c, 3, 3, generator=g) / (3 * c ** 0.5)).to(dev)
    bias = torch.randn(co, generator=g).to(dev)
    oh, ow = R.out_hw(h, w)
    with torch.no_grad():
        dense = ops._conv_s2_bf16x1_impl(ops.to_nhwc(xc.to(dev)), wc, bias, 2, 0.2)
        xs = LP.poisoned_slice(xc, 96, 16, dev)
        out = LP.canary_slice(n, co, oh, ow, 72, 4, dev)
        assert ops.nhwc_ld(xs) == 96 and ops.nhwc_ld(out) == 72
        got = ops._conv_s2_bf16x1_impl(xs, wc, bias, 2, 0.2, out=out)
    assert got is out
    LP.check_slice(xs); LP.check_slice(out, written=True)
    assert torch.equal(out.cpu(), dense.cpu())
    # the gradient: dy [1, 64, oh, ow] -> dx [1, 64, h, w]
    dyc = torch.randn(n, co, oh, ow, generator=g) * 1.5 + 0.3
    with torch.no_grad():
        dense = ops._conv_dgrad_s2_bf16x1_impl(ops.to_nhwc(dyc.to(dev)), wc, h, w, 0, c)
        dys = LP.poisoned_slice(dyc, 80, 8, dev)
        out = LP.canary_slice(n, c, h, w, 72, 4, dev)
        got = ops._conv_dgrad_s2_bf16x1_impl(dys, wc, h, w, 0, c, out=out)
        assert got is out
        LP.check_slice(dys); LP.check_slice(out, written=True)
        assert torch.equal(out.cpu(), dense.cpu())
        # one class at a time: exactly its parity positions are written
        for k, (py, px, taps) in enumerate(ops._s2_classes()):
            alone = LP.canary_slice(n, c, h, w, 72, 4, dev)
            gh, gw = (h - py + 1) // 2, (w - px + 1) // 2
            wpk, kp, kmode = ops._pack(wc, 1, taps, co, co)
            d = ops._conv_desc(ops._at(dys), co, None, 0, (n, oh, ow), wpk.data_ptr(), kp, kmode, None, None, ops._at(alone), c,
                               (gh, gw, h, w), 1, 2, (py, px), taps, 0, 0.0)
            fmt = pkg._lib.call('ssg_conv2d_bf16x1_cls_ok', ctypes.byref(d))
            assert fmt == 1064
            pack = ops._x1_cls_pack(wc, wpk, kp, taps, fmt, 0, c)
            pkg._lib.call('ssg_conv2d_bf16x1_cls_f32', ctypes.byref(d), pkg._lib.ptr(pack), pkg._lib.stream_ptr())
            LP.check_slice(alone)
            written = ~LP.is_canary(alone.cpu())
            want = torch.zeros(n, c, h, w, dtype=torch.bool)
            want[:, :, py::2, px::2] = True
            assert torch.equal(written, want), (py, px)
            assert torch.equal(alone.cpu()[:, :, py::2, px::2], dense.cpu()[:, :, py::2, px::2])


def test_nonfinite_operands_give_the_fp32_kernels_classes(pkg, dev):
    """+-inf, NaN, and two values finite in fp32 of which one (3.4e38) becomes infinite in bf16 and the other (3.39e38) the largest
    finite bf16; weight scale 1e-3.  The set of non-finite outputs is that of ops.conv2d at stride 2, and of its gradient."""
    ops = pkg.ops
    g = torch.Generator().manual_seed(11)
    xc = torch.randn(1, 64, 17, 66, generator=g) * 1.5 + 0.3
    wc = torch.randn(64, 64, 3, 3, generator=g) * 1e-3
    xc[0, 3, 2, 5] = float('inf'); xc[0, 40, 12, 20] = float('nan'); xc[0, 17, 7, 29] = 3.4e38; xc[0, 60, 13, 3] = 3.39e38
    xc[0, 9, 16, 65] = float('-inf')
    xd, wd = ops.to_nhwc(xc.to(dev)), wc.to(dev)
    with torch.no_grad():
        y = ops._conv_s2_bf16x1_impl(xd, wd, None, 0, 0.0).cpu()
        y32 = ops.conv2d(xd, wd, stride=2, padding=1).cpu()
    fin = torch.isfinite(y32)
    assert torch.equal(torch.isfinite(y), fin) and torch.equal(torch.isnan(y), torch.isnan(y32))
    assert 0 < (~fin).sum().item() < fin.numel()
    big = xc.clone(); big[~torch.isfinite(big)] = 0.0
    exact = R.conv64(xc, wc)
    assert ((y.double() - exact).abs()[fin] <= (R.conv_bound(big, wc) + 1e-3)[fin]).all()
    # the gradient: the same poison in dy [1, 64, 9, 33] -> dx [1, 64, 18, 66]
    dyc = torch.randn(1, 64, 9, 33, generator=g) * 1.5 + 0.3
    dyc[0, 3, 2, 5] = float('inf'); dyc[0, 40, 8, 20] = float('nan'); dyc[0, 17, 7, 29] = 3.4e38; dyc[0, 60, 0, 3] = 3.39e38
    dyc[0, 9, 8, 32] = float('-inf')
    dyd = ops.to_nhwc(dyc.to(dev))
    with torch.no_grad():
        dx = ops._conv_dgrad_s2_bf16x1_impl(dyd, wd, 18, 66, 0, 64).cpu()
        dx32 = ops._conv_dgrad_impl(dyd, wd, 2, 1, 18, 66, 0, 64).cpu()
    fin = torch.isfinite(dx32)
    assert torch.equal(torch.isfinite(dx), fin) and torch.equal(torch.isnan(dx), torch.isnan(dx32))
    assert 0 < (~fin).sum().item() < fin.numel()


def test_refused_shapes_launch_nothing(pkg, dev):
    ops, lib = pkg.ops, pkg._lib
    mk = lambda *s: torch.randn(*s, device=dev)
    ops.PROFILE = []
    try:
        for x, w in ((mk(1, 48, 20, 40), mk(64, 48, 3, 3)),          # Cin = 48
                     (mk(1, 64, 20, 32), mk(64, 64, 3, 3)),          # output width 16
                     (mk(1, 64, 20, 40), mk(32, 64, 3, 3))):         # Cout = 32
            assert not ops.conv2d_bf16x1_s2_ok(x, w)
            assert ops._conv_s2_bf16x1_impl(ops.to_nhwc(x), w, None, 0, 0.0) is None
            with pytest.raises(ValueError):
                ops.conv2d_bf16x1_train(x, w, stride=2)
        # gradients: dy channels 48; input width 33 (class px = 1 is 16 wide); 32 rows
        for dy, w, h, wd in ((mk(1, 48, 10, 20), mk(48, 64, 3, 3), 20, 40), (mk(1, 64, 10, 17), mk(64, 64, 3, 3), 20, 33),
                             (mk(1, 64, 10, 20), mk(64, 32, 3, 3), 20, 40)):
            assert ops._conv_dgrad_s2_bf16x1_impl(ops.to_nhwc(dy), w, h, wd, 0, w.shape[1]) is None
        # a unit-stride descriptor is not the stride-2 forward's, a forward descriptor is not a class's
        x, w = mk(1, 64, 20, 40), mk(64, 64, 3, 3)
        d = ops._x1_desc(ops.to_nhwc(x), None, w, None)
        assert lib.call('ssg_conv2d_bf16x1_s2_ok', ctypes.byref(d)) == 0
        assert lib.call('ssg_conv2d_bf16x1_cls_ok', ctypes.byref(d)) == 0
        assert lib.load().ssg_conv2d_bf16x1_s2_f32(ctypes.byref(d), ctypes.c_void_p(16), None) != 0
        assert b'bf16x1 s2' in lib.load().ssg_last_error()
        assert lib.load().ssg_conv2d_bf16x1_cls_f32(ctypes.byref(d), ctypes.c_void_p(16), None) != 0
        assert b'bf16x1 cls' in lib.load().ssg_last_error()
        assert ops.PROFILE == []
        # under ops.conv2d(precision='bf16x1') a refused stride-2 shape runs today's kernel, forward and backward, and never raises
        xg = mk(1, 48, 20, 40).requires_grad_()
        wg = mk(64, 48, 3, 3).requires_grad_()
        ops.conv2d(xg, wg, stride=2, padding=1, precision='bf16x1').sum().backward()
        assert ops.PROFILE and not any('_x1_' in p[0] for p in ops.PROFILE), [p[0] for p in ops.PROFILE]
        with pytest.raises(ValueError):
            ops.conv2d(xg, wg, stride=2, padding=1, precision='bf16')
    finally:
        ops.PROFILE = None
