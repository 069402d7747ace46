"""Reference arithmetic for the stride-2 bf16x1 kernels (csrc/conv_s2_k32_x1.hip): the 3x3 stride-2 pad-1 forward conv and its
input gradient as four output-parity classes.  Plain torch on the CPU, fp64.  Plain helper module (not a conftest), shared by
tests/test_s2_bf16x1_ref.py (CPU rehearsal of the gates) and tests/test_conv_s2_bf16x1_gpu.py.  The kernels round both operands
ONCE to bf16 (bf16x1_ref.rb) and accumulate exact products in fp32; bias and activation are fp32."""
import torch
import torch.nn.functional as F

from bf16x1_ref import BOUND, rb, maxrms, _act

# forward: (N, Cin, Cout, H, W) of the INPUT
FWD_CASES = {
    'one_chunk_odd_partial': (2, 32, 64, 19, 70),       # one chunk; odd H; partial tile rows and columns; batch index
    'ring_wrap_min_width': (1, 96, 128, 18, 34),        # 27 steps so the ring wraps; minimum output width 17
    'three_column_tiles': (1, 64, 192, 16, 66),         # three column tiles; a 1-pixel-wide tile
    'epilogue': (1, 64, 64, 64, 64),                    # bias + LeakyReLU 0.2, and bias alone
    'long_reduction': (1, 256, 64, 16, 64),
}
# input gradient: (N, dy channels = conv Cout, weight in-channels, c_lo, c_hi, h, w of the INPUT)
DGRAD_CASES = {
    'min_width': (1, 64, 64, 0, 64, 18, 34),
    'unequal_class_grids': (2, 32, 64, 0, 64, 21, 71),  # class grids 11 / 10 x 36 / 35; partial tiles
    'ring_wrap_three_tiles': (1, 96, 192, 0, 192, 16, 36),   # ring wrap at 4 taps; 3 steps at 1 tap; three column tiles
    'long_reduction': (1, 256, 64, 0, 64, 16, 64),
    'channel_slice': (1, 64, 128, 64, 128, 18, 36),     # rows [64, 128) of a 128-row transposed weight
    'wide_rows': (1, 32, 128, 0, 128, 16, 34),          # 128 gradient rows: the 128-column tiles
}


def out_hw(h, w):
    return (h - 1) // 2 + 1, (w - 1) // 2 + 1


def _clean(t):
    t[t.abs() < 1e-30] = 0.0
    return t


def make_fwd_case(name, seed=41):
    n, ci, co, h, w = FWD_CASES[name]
    g = torch.Generator().manual_seed(seed + sum(FWD_CASES[name]))
    x = torch.randn(n, ci, h, w, generator=g) * 1.5 + 0.3
    wt = torch.randn(co, ci, 3, 3, generator=g) / (3 * ci ** 0.5)
    return _clean(x), _clean(wt)


def make_dgrad_case(name, seed=43):
    """(dy [N, O, oh, ow], weight [O, I, 3, 3])."""
    n, o, i, c_lo, c_hi, h, w = DGRAD_CASES[name]
    oh, ow = out_hw(h, w)
    g = torch.Generator().manual_seed(seed + sum(DGRAD_CASES[name]))
    dy = torch.randn(n, o, oh, ow, generator=g) * 1.5 + 0.3
    wt = torch.randn(o, i, 3, 3, generator=g) / (3 * o ** 0.5)
    return _clean(dy), _clean(wt)


def conv64(x, w, bias=None, act=None, slope=0.0):
    """act(conv3x3(x, w, stride 2, pad 1) + bias), everything fp64, operands as given."""
    return _act(F.conv2d(x.double(), w.double(), None if bias is None else bias.double(), 2, 1), act, slope)


def conv_ref(x, w, bias=None, act=None, slope=0.0):
    return conv64(rb(x), rb(w), bias, act, slope)


def conv_bound(x, w):
    return BOUND * F.conv2d(x.double().abs(), w.double().abs(), None, 2, 1)


def dgrad64(dy, w, h, wd, c_lo=0, c_hi=None):
    """The autograd gradient of F.conv2d(x, w, stride 2, padding 1) for x [N, I, h, wd], rows [c_lo, c_hi), fp64, operands as given."""
    x = torch.zeros(dy.shape[0], w.shape[1], h, wd, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x, w.double(), None, 2, 1)
    (gx,) = torch.autograd.grad(y, x, dy.double())
    return gx[:, c_lo:c_hi]


def dgrad_ref(dy, w, h, wd, c_lo=0, c_hi=None):
    return dgrad64(rb(dy), rb(w), h, wd, c_lo, c_hi)


def dgrad_bound(dy, w, h, wd, c_lo=0, c_hi=None):
    return BOUND * dgrad64(dy.abs(), w.abs(), h, wd, c_lo, c_hi)


def classes():
    """(py, px, [(ky, kx, dy offset, dx offset)]) of the four output-parity classes: the tap lists of ops._conv_dgrad_impl for a 3x3
    kernel, stride 2, padding 1 -- tap (ky, kx) reaches input row 2 gy + py from output row gy + (py + 1 - ky) / 2."""
    out = []
    for py in range(2):
        for px in range(2):
            taps = [(ky, kx, (py + 1 - ky) // 2, (px + 1 - kx) // 2) for ky in range(3) for kx in range(3)
                    if (py + 1 - ky) % 2 == 0 and (px + 1 - kx) % 2 == 0]
            out.append((py, px, taps))
    return out


def dgrad_by_classes(dy, w, h, wd, c_lo=0, c_hi=None, dtype=torch.float64, drop_tap=None, shift_class=None):
    """The gradient assembled as the kernels do: class (py, px) is a unit-stride conv over dy with its taps, written at stride 2 and
    offset (py, px).  dtype: the accumulation type (fp32 = the kernel's stand-in).  drop_tap = (class index, tap index) leaves a
    tap out; shift_class = class index writes that class at the offset of the next one (both: deliberate faults for the rehearsal)."""
    n, o, oh, ow = dy.shape
    wsel = w[:, c_lo:c_hi].to(dtype)
    dyp = F.pad(dy.to(dtype), (0, 1, 0, 1))
    dx = torch.zeros(n, wsel.shape[1], h, wd, dtype=dtype)
    cls = classes()
    for k, (py, px, taps) in enumerate(cls):
        gh, gw = (h - py + 1) // 2, (wd - px + 1) // 2
        acc = torch.zeros(n, wsel.shape[1], gh, gw, dtype=dtype)
        for t, (ky, kx, oy, ox) in enumerate(taps):
            if drop_tap == (k, t):
                continue
            acc += torch.einsum('nohw,oc->nchw', dyp[:, :, oy:oy + gh, ox:ox + gw], wsel[:, :, ky, kx])
        if shift_class == k:
            py, px = cls[(k + 1) % 4][:2]
            gh2, gw2 = (h - py + 1) // 2, (wd - px + 1) // 2
            acc = acc[:, :, :gh2, :gw2]
        dx[:, :, py::2, px::2][:, :, :acc.shape[2], :acc.shape[3]] = acc
    return dx


def gates(y, y32, ref, exact, bound):
    """The accuracy gates of tests/test_conv_s2_bf16x1_gpu.py on fp64 CPU tensors; returns (b ok, c ok, figures).
      (b) max and rms error of y against `ref` (fp64 on the rounded operands) <= 2 x those of y32 (the fp32-MFMA kernel on the same
          rounded operands), + 1e-6 / 1e-8 as tests/test_conv_bf16x1_gpu.py;
      (c) |y - exact| <= bound + 2 x (max error of y32) + 1e-6 elementwise (exact: fp64 on the operands as given)."""
    em, er = maxrms(y - ref)
    bm, br = maxrms(y32 - ref)
    b_ok = em <= 2.0 * bm + 1e-6 and er <= 2.0 * br + 1e-8
    c_ok = bool(((y - exact).abs() <= bound + 2.0 * bm + 1e-6).all())
    return b_ok, c_ok, (em, er, bm, br)
