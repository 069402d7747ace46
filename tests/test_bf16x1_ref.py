"""CPU rehearsal of the gates the bf16x1 GPU tests set (tests/bf16x1_ref.py): the rounding rule of the reference is the
hardware's, the a-priori bound holds on the test shapes, and a STAND-IN for the kernel -- the same rounded operands convolved in
fp32 on the CPU -- passes every gate, so the caps in tests/test_conv_bf16x1_gpu.py and tests/test_infer_bf16x1_gpu.py do not fail
a correct implementation."""
import pytest
import torch
import torch.nn.functional as F

import bf16x1_ref as R


def test_rb_is_round_to_nearest_even_with_overflow_to_infinity():
    one = 1.0
    ulp = 2.0 ** -7                                      # bf16 spacing in [1, 2)
    cases = [
        (one + ulp / 2, one),                            # tie: 1 has an even significand, 1 + ulp an odd one
        (one + 3 * ulp / 2, one + 2 * ulp),              # tie: up to the even neighbour
        (one + ulp / 2 + 2.0 ** -23, one + ulp),         # just above a tie
        (one + 3 * ulp / 2 - 2.0 ** -23, one + ulp),     # just below a tie
        (-(one + ulp / 2), -one),
        (3.39e38, 3.3895313892515355e38),                # below the halfway point 2^128 - 2^119 = 3.3962e38: the largest finite bf16
        (3.3961e38, 3.3895313892515355e38),
        (3.3962e38, float('inf')),                       # finite in fp32 (max 3.4028e38), infinite after rounding
        (3.4e38, float('inf')),
        (-3.4e38, float('-inf')),
    ]
    x = torch.tensor([c[0] for c in cases], dtype=torch.float32)
    want = torch.tensor([c[1] for c in cases], dtype=torch.float32)
    got = R.rb(x)
    assert torch.equal(got, want), (got.tolist(), want.tolist())
    assert torch.isnan(R.rb(torch.tensor([float('nan')]))).all()
    # the integer statement of the rule on random finite values
    g = torch.Generator().manual_seed(5)
    v = torch.randn(4096, generator=g) * 3
    u = v.view(torch.int32).to(torch.int64) & 0xffffffff
    r = ((u + 0x7fff + ((u >> 16) & 1)) >> 16) << 16
    r = torch.where(r >= 2 ** 31, r - 2 ** 32, r).to(torch.int32).view(torch.float32)
    assert torch.equal(R.rb(v), r)


@pytest.mark.parametrize('name', sorted(R.CASES))
def test_rounding_error_is_inside_the_apriori_bound(name):
    x, w = R.make_case(name)
    err = (R.conv_ref(x, w) - R.conv64(x, w)).abs()
    bound = R.apriori_bound(x, w)
    ratio = (err / bound).max().item()
    print('%s: worst |conv_ref - fp64| / apriori_bound = %.3f' % (name, ratio))
    assert (err <= bound).all()                          # measured: 0.09 (long_reduction) to 0.29 (one_chunk_partial_tiles) of the bound


@pytest.mark.parametrize('name', sorted(R.CASES))
def test_fp32_standin_passes_the_single_conv_gates(name):
    """The stand-in: fp32 convolution of the rounded operands.  Gate (b) compares the kernel with the fp32-MFMA kernel on the same
    operands -- for the stand-in that is itself, so what is checked is gate (c) with the stand-in's own error as the (b) term."""
    x, w = R.make_case(name)
    n, c1, c2, co, h, wd = R.CASES[name]
    g = torch.Generator().manual_seed(9)
    bias = torch.randn(co, generator=g); res = torch.randn(n, co, h, wd, generator=g)
    for act, slope in ((None, 0.0), ('relu', 0.0), ('lrelu', 0.2)):
        y = F.conv2d(R.rb(x), R.rb(w), bias, 1, 1) + res
        y = R._act(y, act, slope)
        e_ref = (y.double() - R.conv_ref(x, w, bias, res, act, slope)).abs()
        e64 = (y.double() - R.conv64(x, w, bias, res, act, slope)).abs()
        assert (e64 <= R.apriori_bound(x, w) + 2.0 * e_ref.max().item() + 1e-6).all()


def _block(cin, planes, seed):
    """Folded tensors of an eval BasicBlock with non-trivial statistics, as `_folded()` computes them (restated in torch)."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for ci, co in ((cin, planes), (planes, planes)):
        w = torch.randn(co, ci, 3, 3, generator=g) / (3 * ci ** 0.5)
        gamma = 0.5 + torch.rand(co, generator=g); beta = torch.randn(co, generator=g) * 0.2
        mean = torch.randn(co, generator=g) * 0.3; var = 0.5 + torch.rand(co, generator=g)
        scale = gamma * torch.rsqrt(var + 1e-5)
        out += [w * scale.view(-1, 1, 1, 1), beta - mean * scale]
    sc = torch.randn(planes, cin, 1, 1, generator=g) / cin ** 0.5 if cin != planes else None
    return tuple(out), sc


@pytest.mark.parametrize('cin,c2,planes', [(64, 0, 128), (32, 64, 64)])
def test_fp32_standin_passes_the_block_gates(cin, c2, planes):
    """Measured at 2 x 20 x 40: stand-in error over reference error 1.000 in max and 1.000 in rms for both blocks, 0.0044 % (64 -> 128)
    and 0.0029 % (32 + 64 -> 64) of the intermediate roundings differ -- against the caps of 1.5 and 1.25 the GPU test sets."""
    folded, sc = _block(cin + c2, planes, 17)
    g = torch.Generator().manual_seed(18)
    x = torch.randn(2, cin, 20, 40, generator=g) * 1.5 + 0.3
    x2 = torch.randn(2, c2, 20, 40, generator=g) if c2 else None
    exact, _ = R.block64(x, x2, folded, sc, rounded=False)
    helper, yh = R.block64(x, x2, folded, sc, rounded=True)
    stand, ys = R.block64(x, x2, folded, sc, rounded=True, conv=lambda a, b: F.conv2d(a, b, None, 1, 1))
    hm, hr = R.maxrms(helper - exact)
    sm, sr = R.maxrms(stand - exact)
    differ = (R.rb(ys.float()) != R.rb(yh.float())).double().mean().item()
    print('block %d+%d -> %d: stand-in / helper error %.3f max, %.3f rms; %.4f %% of intermediate roundings differ'
          % (cin, c2, planes, sm / hm, sr / hr, 100 * differ))
    assert sm <= 1.5 * hm and sr <= 1.25 * hr
    assert differ < 1e-3
