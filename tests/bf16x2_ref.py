"""Reference arithmetic for the opt-in two-term precision 'bf16x2' (csrc/conv_halo_k32_bf16.hip, csrc/conv_wgrad_k32_bf16.hip): plain
torch / numpy on the CPU, fp64.  Plain helper module (not a conftest), shared by tests/test_bf16x2_ref.py (CPU rehearsal of the
gates) and the three GPU files.

The kernels split each operand ONCE into two bf16 terms, v1 = bf16_rne(v), v2 = bf16_rne(v - v1) (the subtraction is exact in
fp32), and keep three of the four products of a pair: x1 w2, x2 w1, x1 w1.  With u = 2^-8 (bf16 unit roundoff): |v2| <= u |v|,
|v - v1 - v2| <= u^2 |v|, |v1| <= (1 + u) |v|, and the dropped part x w - (x1 w1 + x1 w2 + x2 w1) = x2 w2 + x r_w + r_x w - r_x r_w
is bounded by (u^2 + u^2 + u^2 + u^4 [+ second order]) |x w| <= (3 u^2 + 3 u^4) |x w| = BOUND |x w|."""
import numpy as np
import torch
import torch.nn.functional as F

from conv_ref import C_SPLIT, U32

BOUND = 3.0 * 2.0 ** -16 + 3.0 * 2.0 ** -32
BOUND_X1 = 2.0 ** -8 + 2.0 ** -18                  # the one-term form's (tests/bf16x1_ref.py), for the rehearsal's contrast

# forward cases (N, C1, C2, Cout, H, W, act name, ops act code, slope): one K-step with two partial 8 x 32 pixel tiles in each
# direction; three K-steps (an odd count on a three-stage ring) with Cout = 128 (the 512-thread tile); a second input pointer
# with Cout = 192 (the 64-wide tile, three column tiles).  Every case has bias and residual.
FWD_CASES = {
    'k1_c64_9x33': (2, 32, 0, 64, 9, 33, 'relu', 1, 0.0),
    'k3_c128_17x40': (2, 96, 0, 128, 17, 40, 'lrelu', 2, 0.25),
    'two_ptr_c192_9x33': (2, 32, 64, 192, 9, 33, None, 0, 0.0),
}
# input-gradient cases (N, O = channels of dy, I = input channels of the forward conv, c_lo, c_hi, H, W): proper channel windows
DGRAD_CASES = {
    'o32_win64_9x33': (2, 32, 128, 64, 128, 9, 33),
    'o96_win128_17x40': (2, 96, 192, 64, 192, 17, 40),
}
# weight-gradient cases (N, C1, C2, Cout, H, W): N H W <= 2000 keeps the 12-bit class exact (4095 * 2 * 2000 < 2^24)
WGRAD_CASES = {
    'c64_o64_9x33': (2, 64, 0, 64, 9, 33),
    'c64_o128_17x40': (2, 64, 0, 128, 17, 40),
    'two_ptr_o192_9x33': (2, 64, 64, 192, 9, 33),
}


def rb(t):
    """t rounded to bf16 (round to nearest even), widened back to fp32."""
    return t.float().bfloat16().float()


def split2(t):
    """(t1, t2) fp32: t1 = bf16_rne(t), t2 = bf16_rne(t - t1); torch's bf16 rounding, the subtraction in fp32 (exact)."""
    t = t.float()
    t1 = rb(t)
    return t1, rb(t - t1)


def _act(v, act, slope):
    if act == 'relu':
        return v.clamp_min(0)
    if act == 'lrelu':
        return torch.where(v > 0, v, v * slope)
    return v


def _conv(x, w):
    return F.conv2d(x.double(), w.double(), None, 1, 1)


def _epi(v, bias, res, act, slope):
    if bias is not None:
        v = v + bias.double().view(1, -1, 1, 1)
    if res is not None:
        v = v + res.double()
    return _act(v, act, slope)


def conv_exact(x, w, bias=None, res=None, act=None, slope=0.0):
    """act(conv3x3(x, w, pad 1) + bias + res) in fp64 on the operands as given."""
    return _epi(_conv(x, w), bias, res, act, slope)


def conv_quant(x, w, bias=None, res=None, act=None, slope=0.0, terms=('x1w2', 'x2w1', 'x1w1')):
    """The same with the three kept products of the two-term split, in fp64: what the kernel computes up to fp32 accumulation.
    `terms`: the rehearsal drops one to show that the data classes notice."""
    x1, x2 = split2(x)
    w1, w2 = split2(w)
    pairs = {'x1w2': (x1, w2), 'x2w1': (x2, w1), 'x1w1': (x1, w1), 'x2w2': (x2, w2)}
    v = sum(_conv(*pairs[t]) for t in terms)
    return _epi(v, bias, res, act, slope)


def conv_one_term(x, w, bias=None, res=None, act=None, slope=0.0):
    """The one-term ('bf16x1') restatement: a kernel that rounds once must miss the two-term gates."""
    return conv_quant(x, w, bias, res, act, slope, terms=('x1w1',))


def conv_mag(x, w):
    """conv(|x|, |w|) in fp64: the a-priori term."""
    return _conv(x.abs(), w.abs())


def dgrad_weight(w, c_lo, c_hi):
    """The OIHW weight of the conv that IS the input gradient for input channels [c_lo, c_hi) of a 3x3 stride-1 pad-1 conv with
    weight `w` [O, I, 3, 3]: [c_hi - c_lo, O, 3, 3], taps mirrored."""
    return w[:, c_lo:c_hi].transpose(0, 1).flip(2, 3).contiguous()


def _wg(x, dy):
    """dw[o, i, ky, kx] = sum_{n, y, x} dy[n, o, y, x] xpad[n, i, y + ky, x + kx] in fp64."""
    return F.conv2d(x.double().transpose(0, 1), dy.double().transpose(0, 1), None, 1, 1).transpose(0, 1)


def wgrad_exact(x, dy):
    return _wg(x, dy)


def wgrad_quant(x, dy, terms=('x1d2', 'x2d1', 'x1d1')):
    x1, x2 = split2(x)
    d1, d2 = split2(dy)
    pairs = {'x1d2': (x1, d2), 'x2d1': (x2, d1), 'x1d1': (x1, d1)}
    return sum(_wg(*pairs[t]) for t in terms)


def wgrad_one_term(x, dy):
    return wgrad_quant(x, dy, terms=('x1d1',))


def wgrad_mag(x, dy):
    return _wg(x.abs(), dy.abs())


# ---- gates.  The fp32-accumulation gate is the project's own for its split kernels (conv_ref.hard_gate / wgrad_ref.hard_gate with
# the split constant): K (or P) additions of partial sums bounded by mag, one more mag for the second order, C_SPLIT u32 per product
# for the extra additions of a product's terms, `e` epilogue roundings of a value bounded by magt, u32 |ref| for the store.
def conv_acc_gate(K, mag, ref, e=0, magt=None):
    magt = mag if magt is None else magt
    return (K + 1 + C_SPLIT) * U32 * mag + e * U32 * magt + U32 * ref.abs()


def wgrad_acc_gate(P, mag, ref):
    return (P + 1 + C_SPLIT) * U32 * mag + U32 * ref.abs()


# ---- data classes
def small_ints(shape, g, lim=3):
    return torch.randint(-lim, lim + 1, shape, generator=g).float()


def ints12(shape, g):
    """Integers in [-4095, 4095]: every one is exactly v1 + v2 (at most 16 significant bits), v2 != 0 for most."""
    return torch.randint(-4095, 4096, shape, generator=g).float()


def normal(shape, g, scale=1.0):
    t = torch.randn(shape, generator=g) * scale
    t[t.abs() < 1e-30] = 0.0
    return t


def pack_x2(wp, bn):
    """ssg_pack_weights_bf16x2 restated.  wp: fp32 [R, Kp] in kmode 0 with 9 taps (k = (chunk16 * 9 + tap) * 16 + c); returns the
    uint16 array [R / bn][Kp / 32 steps = chunk32 * 9 + tap][2 planes][bn / 16 fragments][64 lanes][8 values]: lane l of fragment j
    holds output channel j * 16 + (l & 15), channels chunk32 * 32 + (l >> 4) * 8 .. + 7; plane 0 = v1, plane 1 = v2."""
    wp = np.asarray(wp, dtype=np.float32)
    R, Kp = wp.shape
    assert R % bn == 0 and Kp % 288 == 0
    nsteps = Kp // 32
    t = torch.from_numpy(wp)
    planes = [p.bfloat16().view(torch.int16).numpy().view(np.uint16) for p in split2(t)]
    out = np.zeros((R // bn, nsteps, 2, bn // 16, 64, 8), dtype=np.uint16)
    for s in range(nsteps):
        chunk32, tap = divmod(s, 9)
        for g in range(4):
            chunk16 = chunk32 * 2 + (g >> 1)
            k0 = (chunk16 * 9 + tap) * 16 + (g & 1) * 8
            for pl in range(2):
                v = planes[pl][:, k0:k0 + 8].reshape(R // bn, bn // 16, 16, 8)       # [tile][fragment j][row in fragment][8]
                out[:, s, pl, :, 16 * g:16 * g + 16, :] = v
    return out


def rms(e):
    return float(e.double().pow(2).mean().sqrt())
