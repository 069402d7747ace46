"""ops._conv_dgrad_bf16x1_impl: the input gradient of a 3x3 stride-1 pad-1 conv on conv_halo_k32_x1_kernel (dy and the transposed
weight rounded once to bf16, fp32 accumulation), at the small shapes of tests/test_wgrad_x1_gpu.py, with a channel slice
[c_lo, c_hi) of a concat input and the residual epilogue.

Gates: integer operands in [-3, 3] -> bit equality with fp64; full-mantissa operands -> against fp64 on the rounded operands
(K + 2) u32 mag + u32 |ref| (K = 9 Cout products per element, one more term for the residual, any summation order), and against
fp64 on the operands as given that plus (2^-8 + 2^-18) sum |dy| |w|.  Where the predicate refuses (a 32-channel slice, a
16-pixel-wide image) the launcher returns None with nothing launched, and _conv_dgrad_impl(precision='bf16x1') runs its
fp32-class kernel, bit for bit."""
import numpy as np
import pytest
import torch

from bn_ref import bf16_rne

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
BOUND = 2.0 ** -8 + 2.0 ** -18
X1_LABELS = ('conv_halo_k32_x1_kernel<128>', 'conv_halo_k32_x1_kernel<64>')

# (N, Cout = dy channels, Cin of the weight, H, W, c_lo, c_hi, residual)
CASES = {
    'w17': (1, 64, 64, 3, 17, 0, 64, False),
    'w33_n3_slice_hi': (3, 128, 128, 5, 33, 64, 128, True),
    'w40_n3_slice_lo': (3, 64, 128, 9, 40, 0, 64, False),
    'w64_res': (1, 128, 64, 2, 64, 0, 64, True),
    'w33_c128_tile': (3, 64, 128, 5, 33, 0, 128, True),
}


def _q(t):
    return torch.from_numpy(bf16_rne(t.float().numpy()).astype(np.float64))


def _data(name, integer):
    n, o, i, h, w, lo, hi, has_res = CASES[name]
    g = torch.Generator().manual_seed(sum(CASES[name][:7]) + (1 if integer else 2))
    if integer:
        mk = lambda *s: torch.randint(-3, 4, s, generator=g).float()
    else:
        def mk(*s):      # full mantissas: the last bit set
            a = torch.randn(*s, generator=g) + 0.1
            return (a.view(torch.int32) | 1).view(torch.float32)
    dy, wt = mk(n, o, h, w), mk(o, i, 3, 3)
    res = mk(n, hi - lo, h, w) if has_res else None
    return dy, wt, res


def _ref(dy, wt, res, lo, hi, rounded):
    f = _q if rounded else (lambda t: t.double())
    shape = (dy.shape[0], hi - lo, dy.shape[2], dy.shape[3])
    ws, ds = f(wt)[:, lo:hi].contiguous(), f(dy)
    ref = torch.nn.grad.conv2d_input(shape, ws, ds, padding=1)
    mag = torch.nn.grad.conv2d_input(shape, ws.abs(), ds.abs(), padding=1)
    if res is not None:
        ref = ref + res.double(); mag = mag + res.double().abs()
    return ref, mag


def _run(pkg, dev, dy, wt, res, lo, hi):
    ops = pkg.ops
    d = ops.to_nhwc(dy.to(dev)); r = ops.to_nhwc(res.to(dev)) if res is not None else None
    wd = wt.to(dev)
    outs = [ops._conv_dgrad_bf16x1_impl(d, wd, dy.shape[2], dy.shape[3], lo, hi, res=r) for _ in range(2)]
    assert outs[0] is not None, 'the bf16x1 input gradient refused a legal shape'
    torch.cuda.synchronize()
    assert torch.equal(outs[0].cpu(), outs[1].cpu()), 'two runs differ'
    return outs[0].cpu().double()


@pytest.mark.parametrize('name', sorted(CASES))
def test_dgrad_x1_case(pkg, dev, name):
    n, o, i, h, w, lo, hi, _ = CASES[name]
    dy, wt, res = _data(name, True)
    got = _run(pkg, dev, dy, wt, res, lo, hi)
    ref, _ = _ref(dy, wt, res, lo, hi, False)
    assert torch.equal(got, ref), 'integer operands: %d elements differ' % int((got != ref).sum())
    dy, wt, res = _data(name, False)
    got = _run(pkg, dev, dy, wt, res, lo, hi)
    ref_r, mag_r = _ref(dy, wt, res, lo, hi, True)
    ref_e, mag_e = _ref(dy, wt, None, lo, hi, False)
    if res is not None:
        ref_e = ref_e + res.double()
    K = 9 * o + (1 if res is not None else 0)
    gate_r = (K + 2) * U32 * mag_r + U32 * ref_r.abs()
    r_rounded = ((got - ref_r).abs() / gate_r).max().item()
    r_exact = ((got - ref_e).abs() / (gate_r + BOUND * mag_e)).max().item()
    print('RATIO dgrad_x1 %-18s rounded=%.3g exact=%.3g' % (name, r_rounded, r_exact))
    assert r_rounded <= 1 and r_exact <= 1, (r_rounded, r_exact)


def test_pack_is_cached_per_slice(pkg, dev):
    ops = pkg.ops
    dy, wt, _ = _data('w33_n3_slice_hi', True)
    wd = wt.to(dev); d = ops.to_nhwc(dy.to(dev))
    ops._conv_dgrad_bf16x1_impl(d, wd, 5, 33, 64, 128)
    ops._conv_dgrad_bf16x1_impl(d, wd, 5, 33, 0, 64)
    keys = [k for k in wd._ssg_pack_bf16x1[1] if isinstance(k, tuple)]
    assert sorted(keys) == [(1, 0, 64, 1064), (1, 64, 64, 1064)]
    first = wd._ssg_pack_bf16x1[1][(1, 64, 64, 1064)]
    ops._conv_dgrad_bf16x1_impl(d, wd, 5, 33, 64, 128)
    assert wd._ssg_pack_bf16x1[1][(1, 64, 64, 1064)] is first
    wd.add_(1.0)                                   # a new version of the weight: the stamp no longer matches
    ops._conv_dgrad_bf16x1_impl(d, wd, 5, 33, 64, 128)
    assert wd._ssg_pack_bf16x1[1][(1, 64, 64, 1064)] is not first


@pytest.mark.parametrize('shape', [(1, 64, 64, 4, 40, 0, 32), (1, 64, 64, 4, 16, 0, 64)], ids=['slice32', 'w16'])
def test_refused_launch_falls_back_to_the_fp32_class_kernel(pkg, dev, shape):
    ops = pkg.ops
    n, o, i, h, w, lo, hi = shape
    g = torch.Generator().manual_seed(3)
    dy = ops.to_nhwc(torch.randn(n, o, h, w, generator=g).to(dev)); wd = torch.randn(o, i, 3, 3, generator=g).to(dev)
    ops.PROFILE = []
    try:
        assert ops._conv_dgrad_bf16x1_impl(dy, wd, h, w, lo, hi) is None
        assert ops.PROFILE == [], 'a refused launcher launched something'
        got = ops._conv_dgrad_impl(dy, wd, 1, 1, h, w, lo, hi, precision='bf16x1')
        labels = [r[0] for r in ops.PROFILE]
    finally:
        ops.PROFILE = None
    assert len(labels) == 1 and labels[0] not in X1_LABELS
    want = ops._conv_dgrad_impl(dy, wd, 1, 1, h, w, lo, hi)
    assert torch.equal(got.cpu(), want.cpu())
