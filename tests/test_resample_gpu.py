"""The memory-bound kernels between the convolutions against tests/resample_ref.py, at the shapes where such kernels go wrong:
csrc/spatial.hip (max pool / unpool / skip-add, bilinear and nearest x2, adaptive average pool) and pixel_gate / spade_modulate of
csrc/pointwise.hip, all through the public ops.  tests/test_resample_ref.py rehearses every gate used here on the CPU: a float32
emulation of each kernel passes it at these very shapes, and each planted defect fails it.

Every gate is one of: exact (bits; NaNs as positions); a rounding count times 2^-24 times a magnitude sum that the fp64 reference
computes (counts derived in resample_ref.py beside K_BIL_FWD / k_bil_bwd and in the *_ref docstrings); or a tolerance that
tests/test_ops_gpu.py already holds for the same op (pixel gate).  No case is filtered by value: the non-finite windows are compared.

* max pool / unpool / skip: y, idx byte for byte, pool backward, unpool forward and backward through the returned idx, and the
  three backward branches of max_pool2x2_skip with the entry point each one launches; inputs carry ties in most windows, 2 % NaN
  and 1 % -inf; the special tensor enumerates ATen's NaN and tie rules with four different argmax bytes in every channel quad.
* bilinear: both forms against the fp64 reference on fp32-formed coordinates, no image-size factor in the gate.
* pixel gate: found dpsi = acc * s * (1 - s) losing 1.3e-3 of its value at psi = 10 to the cancellation in 1 - s (39 x the gate at
  C = 4); the kernel now forms 1 - s as exp(-psi) * s for psi >= 0.

Worst measured error / gate per family on an MI355X (pass: <= 1; the CPU rehearsal's figure in brackets):

    bilinear forward            0.52 gather form, 0.66 streaming form   [0.55, 0.73]
    bilinear backward           0.22 gather form, 0.25 streaming form   [0.22, 0.27]
    max pool / unpool / skip, nearest: exact
    adaptive avgpool            0.61 forward, 0.58 backward             [0.61, 0.58]
    pixel gate                  0.08 y, 0.09 dx, 0.05 dpsi              [0.08, 0.07, 0.03]
    modulate                    0.63 y, 0.99 dx, 1.00 dgamma, dbeta exact   [0.90, 0.99, 1.00]

The file's 94 cases take 4 s on that machine, tests/test_ops_gpu.py 12 s in the same run."""
import numpy as np
import pytest
import torch

import layout_probe as lp
import resample_ref as rr

pytestmark = pytest.mark.gpu


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _np(t):
    return np.ascontiguousarray(t.detach().cpu().contiguous().numpy())


def _report(family, ratios):
    print('RATIO %-28s %s' % (family, '  '.join('%s=%.3f' % kv for kv in sorted(ratios.items()))))


class _Calls(object):
    """Records the entry points the ops launch (ops.call), passing every call through."""

    def __init__(self, monkeypatch, pkg):
        self.names = []
        real = pkg.ops.call

        def spy(name, *a):
            self.names.append(name)
            return real(name, *a)
        monkeypatch.setattr(pkg.ops, 'call', spy)

    def take(self):
        out, self.names = self.names, []
        return out


# ----------------------------------------------------------------------------- max pool / unpool / skip: exact
@pytest.mark.parametrize('shape', rr.POOL_SHAPES + ['special'])
def test_pool_unpool_skip_exact(pkg, dev, shape, monkeypatch):
    ops = pkg.ops
    if shape == 'special':
        x, expected = rr.special_windows()
    else:
        x = rr.pool_input(shape, 11)
    y_ref, k_ref = rr.maxpool_ref(x)                       # the reference, computed once for all checks below
    g = _gen(12)
    dy = torch.randn(y_ref.shape, generator=g); z = torch.randn(y_ref.shape, generator=g)
    du = torch.randn(x.shape, generator=g); ds = torch.randn(x.shape, generator=g)
    dx_ref = rr.scatter_ref(dy.numpy(), k_ref)

    xd = x.to(dev).requires_grad_(True)
    yd, idx = ops.max_pool2x2(xd)
    assert idx.dtype == torch.uint8 and tuple(idx.shape) == k_ref.shape
    assert np.array_equal(_np(idx), k_ref), 'idx differs in %d bytes' % int((_np(idx) != k_ref).sum())
    assert rr.same_bits(_np(yd), y_ref), 'pooled values'
    yd.backward(dy.to(dev))
    assert rr.same_bits(_np(xd.grad), dx_ref), 'pool backward'

    zd = z.to(dev).requires_grad_(True)
    ud = ops.max_unpool2x2(zd, idx)
    ud.backward(du.to(dev))
    assert rr.same_bits(_np(ud), rr.scatter_ref(z.numpy(), k_ref)), 'unpool forward'
    assert rr.same_bits(_np(zd.grad), rr.gather_ref(du.numpy(), k_ref)), 'unpool backward'

    calls = _Calls(monkeypatch, pkg)
    for use in ('y', 'skip', 'both'):
        xs = x.to(dev).requires_grad_(True)
        ys, idx_s, skip = ops.max_pool2x2_skip(xs)
        assert np.array_equal(_np(idx_s), k_ref) and rr.same_bits(_np(ys), y_ref) and rr.same_bits(_np(skip), x.numpy())
        calls.take()
        if use == 'y':
            ys.backward(dy.to(dev))
            want, entry = dx_ref, ['ssg_maxpool2x2_bwd_f32']
        elif use == 'skip':
            skip.backward(ds.to(dev))
            want, entry = ds.numpy(), []
        else:
            torch.autograd.backward([ys, skip], [dy.to(dev), ds.to(dev)])
            want, entry = ds.numpy() + dx_ref, ['ssg_maxpool2x2_bwd_add_f32']            # fp32 dskip + scatter(dy), one add
        assert rr.same_bits(_np(xs.grad), want), 'max_pool2x2_skip backward, %s used' % use
        assert [nm for nm in calls.take() if 'pool' in nm] == entry, 'max_pool2x2_skip backward, %s used' % use

    if shape == 'special':
        # where the gradient lands, stated once more without ATen: the last NaN's position, position 0 for all -inf and +-0 ties
        got = _np(idx)[0, :, 0, :]
        assert np.array_equal(got, expected)
        gx = _np(xd.grad)
        for r in range(expected.shape[0]):
            for c in range(8):
                nm = rr.special_pattern_at(r, c)
                win = gx[0, c, 2 * r:2 * r + 2, :].reshape(4)
                k = {'all nan': 3, '[1, nan, 5, nan]': 3, '[inf, inf, 1, nan]': 3, '[nan, nan, 1, 2]': 1, '[5, nan, nan, 1]': 2,
                     'all -inf': 0, '[0, -0, 0, -0]': 0, '[-0, 0, -0, 0]': 0, 'all equal': 0}.get(nm, int(expected[r, c]))
                assert win[k] == dy[0, c, r, 0].item() and np.count_nonzero(win) == 1, (nm, win)


def test_pool_host_refusals(pkg, dev):
    ops = pkg.ops
    for fn in (ops.max_pool2x2, ops.max_pool2x2_skip):
        for bad in ((1, 4, 3, 4), (1, 4, 4, 3), (1, 6, 4, 4)):             # odd H, odd W, C % 4 != 0
            with pytest.raises(ValueError):
                fn(torch.zeros(bad, device=dev))
    z = torch.zeros(1, 4, 2, 2, device=dev)
    for idx in (torch.zeros((1, 2, 2, 8), dtype=torch.uint8, device=dev), torch.zeros((1, 4, 2, 2), dtype=torch.uint8, device=dev),
                torch.zeros((1, 2, 2, 4), dtype=torch.int32, device=dev)):  # wrong C, NCHW-shaped, wrong dtype
        with pytest.raises(ValueError):
            ops.max_unpool2x2(z, idx)


# ----------------------------------------------------------------------------- bilinear x2
@pytest.mark.parametrize('shape,stream', rr.BIL_CASES)
def test_bilinear_against_fp64_on_fp32_coordinates(pkg, dev, shape, stream):
    n, c, h, w = shape
    assert rr.stream_ok(n, h, w, c) == stream            # the form bilinear_stream_ok picks for this shape (both labels are 'bilinear')
    g = _gen(21)
    x = torch.randn(shape, generator=g); dy = torch.randn(n, c, 2 * h, 2 * w, generator=g)
    xd = x.to(dev).requires_grad_(True)
    yd = pkg.ops.upsample2x_bilinear(xd)
    yd.backward(dy.to(dev))
    r = rr.bilinear_ratios(x.numpy(), dy.numpy(), _np(yd), _np(xd.grad), stream)
    _report('bilinear %s' % ('stream' if stream else 'gather'), r)
    assert r['fwd'] <= 1.0, 'forward %s: error / (%d * 2^-24 * A_abs) = %.3f' % (shape, rr.K_BIL_FWD, r['fwd'])
    assert r['bwd'] <= 1.0, 'backward %s: error / (%d * 2^-24 * A_abs) = %.3f' % (shape, rr.k_bil_bwd(h, w, stream), r['bwd'])


# ----------------------------------------------------------------------------- nearest x2
@pytest.mark.parametrize('shape', rr.NEAREST_SHAPES)
def test_nearest_bitwise(pkg, dev, shape):
    n, c, h, w = shape
    g = _gen(61)
    x = torch.randn(shape, generator=g); dy = torch.randn(n, c, 2 * h, 2 * w, generator=g)
    xd = x.to(dev).requires_grad_(True)
    yd = pkg.ops.upsample2x_nearest(xd)
    yd.backward(dy.to(dev))
    assert rr.same_bits(_np(yd), rr.nearest_ref(x.numpy())), 'nearest forward'
    assert rr.same_bits(_np(xd.grad), rr.nearest_bwd_f32(dy.numpy())), 'nearest backward: (a + b) + (c + d)'


# ----------------------------------------------------------------------------- adaptive average pool
@pytest.mark.parametrize('case', rr.AVG_CASES)
def test_adaptive_avgpool_flat_against_fp64(pkg, dev, case):
    o, (h, w), c = case
    g = _gen(31)
    x = torch.randn(rr.AVG_N, c, h, w, generator=g); dy = torch.randn(rr.AVG_N, c * o * o, generator=g)
    xd = x.to(dev).requires_grad_(True)
    yd = pkg.ops.adaptive_avgpool_flat(xd, o)
    assert tuple(yd.shape) == (rr.AVG_N, c * o * o)       # NCHW-flat: the reference is .view(N, -1) of (N, C, O, O)
    yd.backward(dy.to(dev))
    r = rr.avgpool_ratios(x.numpy(), o, dy.numpy(), _np(yd), _np(xd.grad))
    _report('avgpool', r)
    assert r['fwd'] <= 1.0 and r['bwd'] <= 1.0, (case, r)


# ----------------------------------------------------------------------------- pixel gate
@pytest.mark.parametrize('shape', rr.GATE_CASES)
def test_pixel_gate_against_fp64(pkg, dev, shape, monkeypatch):
    x, psi, dy = rr.gate_inputs(shape, 41)
    alloc = lp.GuardedAllocator().install(monkeypatch, pkg)
    xd = x.to(dev).requires_grad_(True); pd = psi.to(dev).requires_grad_(True)
    yd = pkg.ops.pixel_gate(xd, pd)
    yd.backward(dy.to(dev))
    got = dict(y=_np(yd), dx=_np(xd.grad), dpsi=_np(pd.grad))
    r = rr.pixel_gate_ratios(x.numpy(), psi.numpy(), dy.numpy(), got)
    _report('pixel gate', r)
    assert max(r.values()) <= 1.0, (shape, r)
    # lanes 1..3 of the dpsi pixel quad are zero, and nothing was written outside the tensors
    alloc.check()
    dgs = [a for a in alloc.records if a.c == 1 and a.who == 'backward']
    assert len(dgs) == 1 and dgs[0].ld == 4 and int((dgs[0].payload()[:, 1:] != 0).sum()) == 0
    assert rr.same_bits(_np(dgs[0].payload()[:, 0]).reshape(got['dpsi'].shape), got['dpsi'])


# ----------------------------------------------------------------------------- SPADE modulate
@pytest.mark.parametrize('shape', rr.MOD_CASES)
def test_spade_modulate_against_fp64(pkg, dev, shape):
    c = shape[1]
    x, gb, dy = rr.modulate_inputs(shape, 51)
    xd = x.to(dev).requires_grad_(True); gd = gb.to(dev).requires_grad_(True)
    yd = pkg.ops.spade_modulate(xd, gd)
    yd.backward(dy.to(dev))
    dgb = _np(gd.grad)
    got = dict(y=_np(yd), dx=_np(xd.grad), dgam=dgb[:, :c], dbet=dgb[:, c:])
    r = rr.modulate_ratios(x.numpy(), gb.numpy(), dy.numpy(), got)
    _report('modulate', r)
    assert max(r.values()) <= 1.0, (shape, r)
