"""ops.conv2d_bf16x1 (csrc/conv_halo_k32_bf16.hip): the opt-in one-term bf16 3x3 convolution for inference.  Gates, per case of
tests/bf16x1_ref.py (rehearsed on the CPU in tests/test_bf16x1_ref.py):
  (a) route     the launch is labelled halo_k32_x1; over the file, every tile shape the build instantiates has run;
  (b) accuracy  against the fp64 conv of the bf16-rounded operands: max error <= 2 x that of the fp32-MFMA kernel
                (ops.MFMA_SPLIT = False) on the SAME rounded operands + 1e-6, rms likewise + 1e-8 -- the rule of
                tests/test_split_gpu.py; both kernels see exactly representable products, only the accumulation order differs;
  (c) bound     against the fp64 conv of the UNROUNDED operands: error <= (2^-8 + 2^-18) conv(|x|, |w|) + the term of (b),
                elementwise."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import bf16x1_ref as R
import layout_probe as LP

pytestmark = pytest.mark.gpu

# case name -> (bias and residual?, act name, ops act code, slope)
VARIANTS = [
    ('one_chunk_partial_tiles', False, None, 0, 0.0),
    ('ring_wrap_min_width', False, None, 0, 0.0),
    ('two_pointers_three_tiles', False, None, 0, 0.0),
    ('epilogue', True, 'relu', 1, 0.0),
    ('epilogue', True, 'lrelu', 2, 0.2),
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


def _run_variant(pkg, dev, variant):
    """One launch of the new kernel and one of the fp32-MFMA kernel on the rounded operands; computed once per variant."""
    if variant in _DONE:
        return _DONE[variant]
    name, epi, act, code, slope = variant
    ops = pkg.ops
    n, c1, c2, co, h, w = R.CASES[name]
    xc, wc = R.make_case(name)
    g = torch.Generator().manual_seed(77)
    bias = torch.randn(co, generator=g) if epi else None
    res = torch.randn(n, co, h, w, generator=g) if epi else None
    dv = lambda t: None if t is None else t.to(dev)
    x1, x2 = ops.to_nhwc(xc[:, :c1].to(dev)), (ops.to_nhwc(xc[:, c1:].to(dev)) if c2 else None)
    rd = ops.to_nhwc(res.to(dev)) if epi else None
    wd = wc.to(dev)
    assert ops.conv2d_bf16x1_ok(x1, wd, x2=x2, res=rd)
    y, labels = _profiled(ops, lambda: ops.conv2d_bf16x1(x1, wd, dv(bias), act=code, slope=slope, x2=x2, res=rd))
    xr = R.rb(xc)
    x1r, x2r = ops.to_nhwc(xr[:, :c1].to(dev)), (ops.to_nhwc(xr[:, c1:].to(dev)) if c2 else None)
    wr = R.rb(wc).to(dev)
    y32 = _fp32_mfma(ops, lambda: ops._conv_fwd_impl(x1r, x2r, wr, dv(bias), 1, 1, code, slope, res=rd))
    out = dict(y=y.cpu().double(), y32=y32.cpu().double(), labels=labels,
               ref=R.conv_ref(xc, wc, bias, res, act, slope), exact=R.conv64(xc, wc, bias, res, act, slope), bound=R.apriori_bound(xc, wc))
    _DONE[variant] = out
    return out


@pytest.mark.parametrize('variant', VARIANTS, ids=lambda v: '%s-%s' % (v[0], v[2]))
def test_single_conv_route_accuracy_and_bound(pkg, dev, variant):
    r = _run_variant(pkg, dev, variant)
    co = R.CASES[variant[0]][3]
    want = 'conv_halo_k32_x1_kernel<%d>' % (128 if co % 128 == 0 else 64)
    assert r['labels'] == [want], r['labels']                                            # (a)
    em, er = R.maxrms(r['y'] - r['ref'])
    bm, br = R.maxrms(r['y32'] - r['ref'])
    print('%s: x1 max %.3e rms %.3e | fp32 MFMA on the rounded operands max %.3e rms %.3e | worst error / a-priori bound %.3f'
          % (variant[0], em, er, bm, br, ((r['y'] - r['exact']).abs() / r['bound']).max().item()))
    assert em <= 2.0 * bm + 1e-6, (em, bm)                                               # (b)
    assert er <= 2.0 * br + 1e-8, (er, br)
    assert ((r['y'] - r['exact']).abs() <= r['bound'] + 2.0 * bm + 1e-6).all()            # (c)


def test_every_instantiated_tile_shape_ran(pkg, dev):
    seen = set()
    for v in VARIANTS:
        seen |= set(_run_variant(pkg, dev, v)['labels'])
    assert seen == set(pkg.ops._X1_LABELS.values()), seen


def test_channel_slices_of_wider_tensors(pkg, dev):
    """x, res and out are channel slices (ld > C) of canary-filled, guarded buffers: same bits as on dense tensors, neighbouring
    lanes and guard bands untouched, every element of the destination written."""
    ops = pkg.ops
    n, c, co, h, w = 1, 64, 64, 9, 20
    g = torch.Generator().manual_seed(5)
    xc = torch.randn(n, c, h, w, generator=g) * 1.5 + 0.3
    wc = (torch.randn(co, c, 3, 3, generator=g) / (3 * c ** 0.5)).to(dev)
    rc = torch.randn(n, co, h, w, generator=g)
    bias = torch.randn(co, generator=g).to(dev)
    dense = ops.conv2d_bf16x1(ops.to_nhwc(xc.to(dev)), wc, bias, act=1, res=ops.to_nhwc(rc.to(dev)))
    xs = LP.poisoned_slice(xc, 96, 16, dev)
    rs = LP.poisoned_slice(rc, 80, 8, dev)
    out = LP.canary_slice(n, co, h, w, 72, 4, dev)
    assert ops.nhwc_ld(xs) == 96 and ops.nhwc_ld(rs) == 80 and ops.nhwc_ld(out) == 72
    with torch.no_grad():
        got = ops._conv_bf16x1_impl(xs, wc, bias, 1, 0.0, res=rs, out=out)
    assert got is out
    LP.check_slice(xs); LP.check_slice(rs); LP.check_slice(out, written=True)
    assert torch.equal(out.cpu(), dense.cpu())


def test_nonfinite_operands_give_the_fp32_kernels_classes(pkg, dev):
    """+inf, NaN, and two values finite in fp32 of which one (3.4e38, beyond 2^128 - 2^119 = 3.3962e38) becomes infinite in bf16 and
    the other (3.39e38) the largest finite bf16; weight scale 1e-3.  The set of non-finite outputs is ops.conv2d's, every other
    element meets (c)."""
    ops = pkg.ops
    g = torch.Generator().manual_seed(11)
    clean = torch.randn(1, 64, 16, 32, generator=g) * 1.5 + 0.3
    wc = torch.randn(64, 64, 3, 3, generator=g) * 1e-3
    xc = clean.clone()
    xc[0, 3, 2, 5] = float('inf'); xc[0, 40, 12, 20] = float('nan'); xc[0, 17, 7, 29] = 3.4e38; xc[0, 60, 13, 3] = 3.39e38
    wd = wc.to(dev)
    y = ops.conv2d_bf16x1(ops.to_nhwc(xc.to(dev)), wd).cpu().double()
    y32 = ops.conv2d(ops.to_nhwc(xc.to(dev)), wd, padding=1).cpu().double()
    assert torch.equal(torch.isfinite(y), torch.isfinite(y32))
    fin = torch.isfinite(y32)
    assert 0 < (~fin).sum().item() < fin.numel()
    # the (b) term from the same shape without the poison
    xr, wr = ops.to_nhwc(R.rb(clean).to(dev)), R.rb(wc).to(dev)
    bm, _ = R.maxrms(_fp32_mfma(ops, lambda: ops._conv_fwd_impl(xr, None, wr, None, 1, 1, 0, 0.0)).cpu().double() - R.conv_ref(clean, wc))
    exact = F.conv2d(xc.double(), wc.double(), None, 1, 1)
    big = xc.clone(); big[~torch.isfinite(big)] = 0.0
    bound = R.apriori_bound(big, wc)
    assert torch.isfinite(exact[fin]).all()
    assert ((y - exact).abs()[fin] <= (bound + 2.0 * bm + 1e-6)[fin]).all()


def test_refusals_launch_nothing(pkg, dev):
    ops, lib = pkg.ops, pkg._lib
    mk = lambda *s: torch.randn(*s, device=dev)
    ops.PROFILE = []
    try:
        for x, w in ((mk(1, 48, 20, 20), mk(64, 48, 3, 3)),          # Cin = 48
                     (mk(1, 64, 20, 16), mk(64, 64, 3, 3)),          # W = 16
                     (mk(1, 64, 20, 20), mk(32, 64, 3, 3))):         # Cout = 32
            assert not ops.conv2d_bf16x1_ok(x, w)
            with pytest.raises(ValueError):
                ops.conv2d_bf16x1(x, w)
        # stride 2: conv2d_bf16x1 has no stride argument; the descriptor of a legal launch with in_sy = in_sx = 2 is refused on the host
        x, w = mk(1, 64, 20, 20), mk(64, 64, 3, 3)
        assert ops.conv2d_bf16x1_ok(x, w)
        d = ops._x1_desc(ops.to_nhwc(x), None, w, None)
        d.in_sy = d.in_sx = 2; d.GH = d.GW = d.OH = d.OW = 10
        assert lib.call('ssg_conv2d_bf16x1_ok', ctypes.byref(d)) == 0
        assert lib.load().ssg_conv2d_bf16x1_f32(ctypes.byref(d), ctypes.c_void_p(16), None) != 0
        assert b'bf16x1' in lib.load().ssg_last_error()
        xg = mk(1, 64, 20, 20).requires_grad_()
        with torch.enable_grad(), pytest.raises(RuntimeError, match='inference-only'):
            ops.conv2d_bf16x1(xg, w)
        with torch.no_grad():
            assert ops.conv2d_bf16x1(xg, w).requires_grad is False
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            ops.conv2d_bf16x1(torch.randn(1, 64, 20, 20), torch.randn(64, 64, 3, 3))
        assert [p[0] for p in ops.PROFILE] == ['conv_halo_k32_x1_kernel<64>']      # the one legal call under no_grad, nothing else
    finally:
        ops.PROFILE = None
