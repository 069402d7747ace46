"""CPU rehearsal of the gates of tests/test_conv_bf16x2_gpu.py, tests/test_wgrad_x2_gpu.py and tests/test_train_x2_gpu.py: the
data classes tell a correct two-term kernel from a one-term kernel and from a kernel that drops either cross product.  No library,
no GPU: fp64 references of tests/bf16x2_ref.py against each other."""
import pytest
import torch
import torch.nn.functional as F

import bf16x2_ref as R

N, C, CO, H, W = 2, 96, 64, 9, 33        # K = 864, the longest reduction of the GPU cases


def _g(seed):
    return torch.Generator().manual_seed(seed)


def test_split2_is_exact_for_16_bit_integers_and_bounded_for_full_mantissas():
    v = torch.arange(-65535, 65536).float()
    v1, v2 = R.split2(v)
    assert torch.equal(v1 + v2, v)
    twelve = v[(v.abs() <= 4095)]
    assert (R.split2(twelve)[1] != 0).float().mean().item() > 0.8          # the second term matters for most 12-bit values
    x = R.normal((1 << 16,), _g(1))
    x1, x2 = R.split2(x)
    assert ((x.double() - x1.double() - x2.double()).abs() <= 2.0 ** -16 * x.double().abs()).all()
    assert (x2.abs() <= 2.0 ** -8 * x.abs()).all()


def test_product_bound_over_random_pairs():
    g = _g(2)
    x, w = R.normal((1 << 20,), g), R.normal((1 << 20,), g)
    x1, x2 = (t.double() for t in R.split2(x))
    w1, w2 = (t.double() for t in R.split2(w))
    kept = x1 * w1 + x1 * w2 + x2 * w1
    exact = x.double() * w.double()
    rel = ((kept - exact).abs() / exact.abs().clamp_min(1e-300)).max().item()
    assert rel <= R.BOUND, rel
    assert ((x1 * w1 - exact).abs() / exact.abs().clamp_min(1e-300)).max().item() > 16 * R.BOUND      # one term is far outside


@pytest.mark.parametrize('side', ['x12', 'w12'])
def test_two_term_integers_conv_quantised_is_exact_one_term_and_dropped_terms_are_not(side):
    g = _g(3)
    x = R.ints12((N, C, H, W), g) if side == 'x12' else R.small_ints((N, C, H, W), g, 2)
    w = R.small_ints((CO, C, 3, 3), g, 2) if side == 'x12' else R.ints12((CO, C, 3, 3), g)
    exact = R.conv_exact(x, w)
    assert exact.abs().max().item() < 2 ** 24 and R.conv_mag(x, w).max().item() < 2 ** 24
    assert torch.equal(R.conv_quant(x, w), exact)
    assert not torch.equal(R.conv_one_term(x, w), exact)
    # the cross product that carries this side's second term is the one whose loss shows here; the other shows on the other side
    dropped = ('x1w2', 'x1w1') if side == 'x12' else ('x2w1', 'x1w1')
    assert not torch.equal(R.conv_quant(x, w, terms=dropped), exact)


@pytest.mark.parametrize('side', ['x12', 'd12'])
def test_two_term_integers_wgrad_quantised_is_exact_one_term_and_dropped_terms_are_not(side):
    g = _g(4)
    n, c, co, h, w = 2, 64, 64, 9, 33
    x = R.ints12((n, c, h, w), g) if side == 'x12' else R.small_ints((n, c, h, w), g, 2)
    d = R.small_ints((n, co, h, w), g, 2) if side == 'x12' else R.ints12((n, co, h, w), g)
    exact = R.wgrad_exact(x, d)
    assert R.wgrad_mag(x, d).max().item() < 2 ** 24
    assert torch.equal(R.wgrad_quant(x, d), exact)
    assert not torch.equal(R.wgrad_one_term(x, d), exact)
    dropped = ('x1d2', 'x1d1') if side == 'x12' else ('x2d1', 'x1d1')
    assert not torch.equal(R.wgrad_quant(x, d, terms=dropped), exact)


def test_full_mantissa_conv_quantised_inside_the_bound_one_term_outside():
    g = _g(5)
    x = R.normal((N, C, H, W), g)
    w = R.normal((CO, C, 3, 3), g, (9 * C) ** -0.5)
    exact, mag = R.conv_exact(x, w), R.conv_mag(x, w)
    eq = (R.conv_quant(x, w) - exact).abs()
    assert (eq <= R.BOUND * mag).all()
    e1 = (R.conv_one_term(x, w) - exact).abs()
    assert (e1 > R.BOUND * mag).float().mean().item() > 0.5
    print('quantised / bound: max %.3f; one-term / bound: max %.1f' % ((eq / (R.BOUND * mag)).max().item(), (e1 / (R.BOUND * mag)).max().item()))


def test_full_mantissa_wgrad_quantised_inside_the_bound_one_term_outside():
    g = _g(6)
    x = R.normal((2, 64, 9, 33), g)
    d = R.normal((2, 64, 9, 33), g)
    exact, mag = R.wgrad_exact(x, d), R.wgrad_mag(x, d)
    assert ((R.wgrad_quant(x, d) - exact).abs() <= R.BOUND * mag).all()
    assert ((R.wgrad_one_term(x, d) - exact).abs() > R.BOUND * mag).float().mean().item() > 0.5


def test_dgrad_weight_is_the_input_gradient():
    g = _g(7)
    x = R.normal((1, 8, 5, 6), g).double().requires_grad_()
    w = R.normal((4, 8, 3, 3), g).double()
    dy = R.normal((1, 4, 5, 6), g).double()
    F.conv2d(x, w, None, 1, 1).backward(dy)
    got = F.conv2d(dy, R.dgrad_weight(w, 2, 6), None, 1, 1)
    assert torch.allclose(got, x.grad[:, 2:6], rtol=1e-12, atol=1e-12)


def _block(x, w1, w2, conv):
    """relu(conv(relu(conv(x, w1)), w2) + x): the data flow of a BasicBlock without its batch norms, intermediate stored as fp32."""
    y = conv(x, w1).clamp_min(0).float()
    return (conv(y, w2) + x.double()).clamp_min(0)


@pytest.mark.parametrize('seed', [11, 12])
def test_block_rms_ratio_two_term_against_one_term(seed):
    """The module-level gate: RMS difference from the exact block under the two-term products <= 1/16 of that under one term
    (theory ~2^-8; the slack is for an isolated ReLU flip)."""
    g = _g(seed)
    c = 64
    x = R.normal((2, c, 20, 24), g)
    w1 = R.normal((c, c, 3, 3), g, (9 * c) ** -0.5)
    w2 = R.normal((c, c, 3, 3), g, (9 * c) ** -0.5)
    exact = _block(x, w1, w2, R.conv_exact)
    r2 = R.rms(_block(x, w1, w2, R.conv_quant) - exact)
    r1 = R.rms(_block(x, w1, w2, R.conv_one_term) - exact)
    print('block rms: two-term %.3e one-term %.3e ratio %.5f' % (r2, r1, r2 / r1))
    assert r2 <= r1 / 16


def test_pack_restatement_layout():
    """pack_x2 places (row, k) where the kernel's fragment read expects it: lane l of fragment j = row j*16 + (l & 15), k-group l >> 4."""
    R_, Kp, bn = 128, 288, 64
    wp = torch.arange(R_ * Kp).float().reshape(R_, Kp).numpy() % 251           # small integers: plane 0 holds them, plane 1 zeros
    out = R.pack_x2(wp, bn)
    assert out.shape == (2, 9, 2, 4, 64, 8) and not out[:, :, 1].any()
    import numpy as np
    vals = torch.from_numpy(out[:, :, 0].astype(np.int16)).view(torch.bfloat16).float().numpy()
    tile, s, j, l, e = 1, 4, 2, 37, 5                                            # tap 4, chunk32 0
    row, g = tile * bn + j * 16 + (l & 15), l >> 4
    k = ((g >> 1) * 9 + s) * 16 + (g & 1) * 8 + e
    assert vals[tile, s, j, l, e] == wp[row, k]
