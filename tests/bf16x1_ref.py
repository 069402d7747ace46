"""Reference arithmetic for the opt-in bf16 inference convolution (csrc/conv_halo_k32_bf16.hip, ops.conv2d_bf16x1): plain torch on
the CPU, fp64.  Plain helper module (not a conftest), shared by tests/test_bf16x1_ref.py (CPU rehearsal of the gates) and the two
GPU files.  The kernel rounds x, x2 and the weights ONCE to bf16 (round to nearest even) and accumulates exact products in fp32;
bias, residual and activation are fp32."""
import torch
import torch.nn.functional as F

# unit roundoff of bf16 is 2^-9 per operand: |rb(x) rb(w) - x w| <= ((1 + 2^-9)^2 - 1) |x w| = (2^-8 + 2^-18) |x w|
BOUND = 2.0 ** -8 + 2.0 ** -18

# (N, C1, C2, Cout, H, W): the smallest shapes at which each mechanism of the kernel can break
CASES = {
    'one_chunk_partial_tiles': (2, 32, 0, 64, 20, 40),      # one chunk; partial tile rows and columns; batch index
    'ring_wrap_min_width': (1, 96, 0, 128, 9, 17),          # 27 steps so the ring wraps; minimum width; one spill row
    'two_pointers_three_tiles': (2, 32, 64, 192, 16, 33),   # pointer switch at a chunk boundary; three column tiles; 1-pixel-wide tile
    'epilogue': (1, 64, 0, 64, 32, 32),                     # bias + residual + ReLU / leaky ReLU
    'long_reduction': (1, 256, 0, 64, 8, 32),
}


def make_case(name, seed=31):
    """(x [N, C1 + C2, H, W], w [Cout, C1 + C2, 3, 3]) fp32: randn * 1.5 + 0.3 inputs and randn / (3 sqrt(Cin)) weights as in
    tests/test_split_gpu.py; no subnormals."""
    n, c1, c2, co, h, w = CASES[name]
    g = torch.Generator().manual_seed(seed + sum(CASES[name]))
    x = torch.randn(n, c1 + c2, h, w, generator=g) * 1.5 + 0.3
    wt = torch.randn(co, c1 + c2, 3, 3, generator=g) / (3 * (c1 + c2) ** 0.5)
    for t in (x, wt):
        t[t.abs() < 1e-30] = 0.0
    return x, wt


def rb(t):
    """t rounded to bf16 (round to nearest even), widened back to fp32."""
    return t.float().bfloat16().float()


def _act(v, act, slope):
    if act == 'relu':
        return v.clamp_min(0)
    if act == 'lrelu':
        return torch.where(v > 0, v, v * slope)
    return v


def conv64(x, w, bias=None, res=None, act=None, slope=0.0):
    """act(conv3x3(x, w, pad 1) + bias + res), everything fp64, operands as given."""
    v = F.conv2d(x.double(), w.double(), None if bias is None else bias.double(), 1, 1)
    if res is not None:
        v = v + res.double()
    return _act(v, act, slope)


def conv_ref(x, w, bias=None, res=None, act=None, slope=0.0):
    """The fp64 conv of the bf16-rounded operands, bias / res / act in fp64: what the kernel computes up to fp32 accumulation."""
    return conv64(rb(x), rb(w), bias, res, act, slope)


def apriori_bound(x, w):
    """(2^-8 + 2^-18) * conv(|x|, |w|) in fp64: the largest possible effect of rounding both operands of every product."""
    return BOUND * F.conv2d(x.double().abs(), w.double().abs(), None, 1, 1)


def block64(x, x2, folded, sc_weight, rounded, conv=None):
    """Eval-mode BasicBlock on the four folded tensors of the module's own `_folded()` (w1', b1', w2', b2'; CPU copies) and its 1x1
    shortcut weight (or None): relu(conv(y, w2') + b2' + r), y = relu(conv(cat(x, x2), w1') + b1'), r = shortcut(cat(x, x2)).
    `rounded`: round where the device path rounds -- x, x2, the folded 3x3 weights, and the intermediate y (an fp32 tensor on the
    device, rounded again as conv2's operand).  The 1x1 shortcut is never rounded.  `conv(x, w)` (default: fp64) does the two 3x3
    products; tests pass an fp32 one as the kernel's stand-in."""
    w1, b1, w2, b2 = folded
    q = rb if rounded else (lambda t: t)
    conv = conv or (lambda a, b: F.conv2d(a.double(), b.double(), None, 1, 1))
    xin = x if x2 is None else torch.cat([x, x2], 1)
    y = (conv(q(xin), q(w1)).double() + b1.double().view(1, -1, 1, 1)).clamp_min(0)
    r = xin.double() if sc_weight is None else F.conv2d(xin.double(), sc_weight.double())
    yq = q(y.float()) if rounded else y
    out = (conv(yq, q(w2)).double() + b2.double().view(1, -1, 1, 1) + r).clamp_min(0)
    return out, y


def maxrms(e):
    e = e.double().abs()
    return e.max().item(), e.pow(2).mean().sqrt().item()
