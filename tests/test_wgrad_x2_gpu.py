"""ssg_conv2d_wgrad_bf16x2_f32 (csrc/conv_wgrad_k32_bf16.hip, kernel id 92) through the C-ABI: the two-term weight gradient of the
3x3 stride-1 pad-1 conv against tests/bf16x2_ref.py (rehearsed in tests/test_bf16x2_ref.py).

Per case (N H W <= 2000, every pixel stride wider than its channels, dw and the workspace NaN-filled, two runs with the same bits):
  (1) small integers in both operands                                   -> equal to fp64;
  (2) 12-bit integers in x and integers in [-2, 2] in dout, and the other way round -> equal to fp64 (4095 * 2 * 2000 < 2^24);
  (3) N(0, 1) operands -> within the fp32-accumulation gate (wgrad_ref.hard_gate's form with the split constant) of the quantised
      reference, and within that gate + (3 * 2^-16 + 3 * 2^-32) sum |x| |dout| of the exact one;
  (4) +inf, NaN, 3.39e38 in x and in dout -> the NaN / inf / finite pattern of the fp32-class kernel on the same buffers.
Refusals return a status and write nothing."""
import ctypes as C

import numpy as np
import pytest
import torch

import bf16x2_ref as R
import layout_probe as LP

pytestmark = pytest.mark.gpu
NAN = float('nan')


def _g(seed):
    return torch.Generator().manual_seed(seed)


class _Launch(object):
    """The descriptor of ops._conv_wgrad_bf16x1_impl on channel slices of canary-filled buffers; dw and the workspace NaN-filled."""

    def __init__(self, pkg, dev, x, c1, dy, stride=1, entry='ssg_conv2d_wgrad_bf16x2'):
        ops, lib = pkg.ops, pkg._lib
        self.ops, self.lib, self.entry = ops, lib, entry
        n, ci, h, w = x.shape
        co = dy.shape[1]
        c2 = ci - c1
        self.x1 = LP.poisoned_slice(x[:, :c1].contiguous(), c1 + 32, 16, dev)
        self.x2 = LP.poisoned_slice(x[:, c1:].contiguous(), c2 + 16, 8, dev) if c2 else None
        self.dy = LP.poisoned_slice(dy, co + 16, 8, dev)
        self.shape = (co, ci, 3, 3)
        self.d = ops._wgrad_desc(self.x1, c1, self.x2, c2, self.dy, self.shape, stride, ops._X1_TAPS)
        self.dw = torch.full(self.shape, NAN, device=dev)
        self.d.dw_oihw = self.dw.data_ptr()
        self.d.flags = 1
        self.ws_bytes = lib.call(entry + '_workspace_bytes', C.byref(self.d))
        self.ws = torch.full((max(self.ws_bytes, 16) // 4 + 64,), NAN, device=dev)
        self.d.ws = self.ws.data_ptr(); self.d.ws_bytes = self.ws_bytes

    def run(self):
        runs = []
        for _ in range(2):
            self.dw.fill_(NAN); self.ws.fill_(NAN)
            self.lib.call(self.entry + '_f32', C.byref(self.d), self.ops.stream_ptr())
            runs.append(self.dw.cpu())
            assert bool(torch.isnan(self.ws[self.ws_bytes // 4:]).all().item()), 'written past the queried workspace'
        for t in (self.x1, self.x2, self.dy):
            if t is not None:
                LP.check_slice(t)
        assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32)), 'two runs differ'
        return runs[0].double()


def _x2_launch(pkg, dev, x, c1, dy):
    L = _Launch(pkg, dev, x, c1, dy)
    assert pkg._lib.call('ssg_conv2d_wgrad_bf16x2_ok', C.byref(L.d)) == 1
    assert pkg._lib.call('ssg_conv2d_wgrad_bf16x2_kernel_id', C.byref(L.d)) == 92
    assert L.ws_bytes > 0 and L.ws_bytes == pkg._lib.call('ssg_conv2d_wgrad_bf16x1_workspace_bytes', C.byref(L.d))    # the x1 plan
    return L


@pytest.mark.parametrize('kind', ['ints', 'x12', 'd12', 'normal'])
@pytest.mark.parametrize('name', sorted(R.WGRAD_CASES))
def test_weight_gradient(pkg, dev, name, kind):
    n, c1, c2, co, h, w = R.WGRAD_CASES[name]
    P = n * h * w
    assert P <= 2000
    g = _g(500 + len(name) + len(kind))
    xs, ds = (n, c1 + c2, h, w), (n, co, h, w)
    if kind == 'ints':
        x, d = R.small_ints(xs, g), R.small_ints(ds, g)
    elif kind == 'x12':
        x, d = R.ints12(xs, g), R.small_ints(ds, g, 2)
    elif kind == 'd12':
        x, d = R.small_ints(xs, g, 2), R.ints12(ds, g)
    else:
        x, d = R.normal(xs, g), R.normal(ds, g)
    dw = _x2_launch(pkg, dev, x, c1, d).run()
    exact = R.wgrad_exact(x, d)
    if kind != 'normal':
        assert R.wgrad_mag(x, d).max().item() < 2 ** 24
        bad = (dw != exact).nonzero()
        assert not len(bad), '%s %s: %d elements differ from fp64, first %s: %r != %r' % (
            name, kind, len(bad), tuple(bad[0].tolist()), dw[tuple(bad[0])].item(), exact[tuple(bad[0])].item())
        return
    quant, mag = R.wgrad_quant(x, d), R.wgrad_mag(x, d)
    gate = R.wgrad_acc_gate(P, mag, quant)
    rq = ((dw - quant).abs() / gate).max().item()
    re = ((dw - exact).abs() / (gate + R.BOUND * mag)).max().item()
    print('RATIO wgrad %s P=%d: |got - quantised| / gate max %.4f; |got - exact| / (gate + bound) max %.4f; |got - exact| / bound max %.4f'
          % (name, P, rq, re, ((dw - exact).abs() / (R.BOUND * mag)).max().item()))
    assert rq <= 1 and re <= 1, (rq, re)


@pytest.mark.parametrize('name', ['two_ptr_o192_9x33', 'c64_o128_17x40'], ids=['nj2_concat', 'nj4'])
def test_bf16_operands_give_the_one_term_kernels_result(pkg, dev, name):
    """The two-term kernel is the one-term kernel plus two sweeps of small terms.  With N(0, 1) operands rounded to bf16 and back,
    split2's second term v - bf16(v) is exactly zero, the sweeps x1 d2 and x2 d1 add zeros, and ssg_conv2d_wgrad_bf16x1 and
    ..._bf16x2 on the same descriptor and buffers (one plan, one workspace size) return EQUAL values (compared as floats: an
    accumulator of -0 may come back +0).  No reference is involved.  NJ = 2 (Cout 192, through the concat) and NJ = 4 (Cout 128)."""
    n, c1, c2, co, h, w = R.WGRAD_CASES[name]
    g = _g(800 + len(name))
    x, d = R.rb(R.normal((n, c1 + c2, h, w), g)), R.rb(R.normal((n, co, h, w), g))
    L = _x2_launch(pkg, dev, x, c1, d)
    dw2 = L.run()
    L.entry = 'ssg_conv2d_wgrad_bf16x1'
    assert pkg._lib.call('ssg_conv2d_wgrad_bf16x1_kernel_id', C.byref(L.d)) == 72
    dw1 = L.run()
    assert bool(torch.isfinite(dw1).all().item()) and bool((dw1 != 0).any().item())
    assert torch.equal(dw1, dw2)


@pytest.mark.parametrize('side', ['x', 'dout'])
@pytest.mark.parametrize('value', [float('inf'), float('nan'), 3.39e38], ids=['inf', 'nan', '3.39e38'])
def test_nonfinite_operands_give_the_fp32_kernels_pattern(pkg, dev, side, value):
    n, c1, c2, co, h, w = R.WGRAD_CASES['c64_o64_9x33']
    g = _g(600)
    x, d = R.normal((n, c1, h, w), g), R.normal((n, co, h, w), g, 0.25)
    (x if side == 'x' else d)[1, 9, 4, 20] = value
    dw = _x2_launch(pkg, dev, x, c1, d).run()
    L32 = _Launch(pkg, dev, x, c1, d, entry='ssg_conv2d_wgrad')
    dw32 = L32.run()
    for pred in (torch.isnan, torch.isposinf, torch.isneginf):
        assert torch.equal(pred(dw), pred(dw32)), pred.__name__
    fin = torch.isfinite(dw32)
    assert fin.any()
    if value != 3.39e38:
        assert (~fin).any()
    xf, df = x.clone(), d.clone()
    if value != 3.39e38:
        (xf if side == 'x' else df)[1, 9, 4, 20] = 0.0
    with np.errstate(all='ignore'):
        exact = R.wgrad_exact(x, d)
    mag = R.wgrad_mag(xf, df)
    gate = R.wgrad_acc_gate(n * h * w, mag, exact.nan_to_num(0.0, 0.0, 0.0)) + R.BOUND * mag
    assert ((dw - exact).abs()[fin] <= gate[fin]).all()


def test_host_refusals_write_nothing(pkg, dev):
    lib = pkg._lib
    g = _g(700)

    def refused(L):
        assert lib.call('ssg_conv2d_wgrad_bf16x2_ok', C.byref(L.d)) == 0
        assert lib.call('ssg_conv2d_wgrad_bf16x2_kernel_id', C.byref(L.d)) < 0
        assert lib.call('ssg_conv2d_wgrad_bf16x2_workspace_bytes', C.byref(L.d)) == 0
        L.d.ws_bytes = 1 << 30                      # not the workspace check: the shape is what is refused
        rc = getattr(lib.load(), 'ssg_conv2d_wgrad_bf16x2_f32')(C.byref(L.d), L.ops.stream_ptr())
        torch.cuda.synchronize()
        assert rc != 0 and b'bf16x2' in lib.load().ssg_last_error()
        assert bool(torch.isnan(L.dw).all().item()) and bool(torch.isnan(L.ws).all().item()), 'a refused call wrote'

    x, d = R.small_ints((1, 64, 8, 40), g), R.small_ints((1, 64, 8, 40), g)
    L = _Launch(pkg, dev, x, 64, d)
    L.d.dx[4] = 1                                                                       # a wrong tap set
    refused(L)
    refused(_Launch(pkg, dev, x, 64, R.small_ints((1, 64, 4, 20), g), stride=2))        # stride 2
    x16 = R.small_ints((1, 64, 8, 16), g)
    refused(_Launch(pkg, dev, x16, 64, R.small_ints((1, 64, 8, 16), g)))                # 16 pixels wide
    refused(_Launch(pkg, dev, x, 64, R.small_ints((1, 96, 8, 40), g)))                  # Cout not a multiple of 64
    L = _x2_launch(pkg, dev, x, 64, d)
    L.d.ws_bytes = L.ws_bytes - 1                                                       # workspace one byte short
    assert getattr(lib.load(), 'ssg_conv2d_wgrad_bf16x2_f32')(C.byref(L.d), L.ops.stream_ptr()) != 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(L.dw).all().item())
    L = _x2_launch(pkg, dev, x, 64, d)                                                  # and the untouched descriptor still runs
    assert torch.equal(L.run(), R.wgrad_exact(x, d))
