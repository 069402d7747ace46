"""CPU rehearsal of tests/resample_ref.py, the oracle of tests/test_resample_gpu.py, before a GPU sees it:

* the references agree with fp64 torch (F.interpolate and autograd of the plain formulas) -- the 'fp32'-coordinate bilinear
  reference is the 'exact' one with a dtype switch, so checking 'exact' against ATen checks its code;
* the selection rule written down for the pool (last NaN, else first maximum) is what stock ATen does on the CPU, in both memory
  formats, on every special window;
* a float32 emulation of each kernel's arithmetic, in the kernel's grouping, passes every gate of the GPU file at every shape of
  the GPU file (a gate the kernel's own arithmetic could exceed would be wrong);
* each planted defect fails its gate at the listed shapes (a gate that lets one through would be too wide).

Worst emulation error / gate over all shapes of a family (pass: <= 1), as printed by this module with -s:

    bilinear forward            0.55 gather shapes, 0.73 streaming shapes     (K = 5)
    bilinear backward, gather   0.22                                          (K = m_x + m_y + 2)
    bilinear backward, stream   0.27                                          (K = m_x + m_y + 3)
    nearest forward / backward  exact
    max pool / unpool / skip    exact
    adaptive avgpool            0.61 forward, 0.58 backward
    pixel gate                  0.08 y, 0.07 dx, 0.03 dpsi
    modulate                    0.90 y, 0.99 dx, 1.00 dgamma (worst-case bounds of two and of one rounding), dbeta exact

Each planted defect misses its gate by a factor of 88 (unrounded coordinate at 128 x 128) to 1e6 (lost band-boundary row).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resample_ref as rr


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _report(family, ratios):
    print('RATIO %-28s %s' % (family, '  '.join('%s=%.3f' % kv for kv in sorted(ratios.items()))))


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(float(np.abs(np.asarray(b)).max()), 1e-300))


# ----------------------------------------------------------------------------- the references against fp64 torch
@pytest.mark.parametrize('hw', [(1, 70), (1, 1), (5, 7), (70, 9)])
def test_bilinear_exact_reference_matches_aten_fp64(hw):
    x = torch.randn(2, 3, *hw, generator=_gen(1), dtype=torch.float64).requires_grad_(True)
    y = F.interpolate(x, scale_factor=2, mode='bilinear', align_corners=True)
    dy = torch.randn(y.shape, generator=_gen(2), dtype=torch.float64)
    y.backward(dy)
    yr, ya = rr.bilinear_ref(x.detach().numpy(), coord='exact')
    dr, da = rr.bilinear_bwd_ref(dy.numpy(), coord='exact')
    assert _rel(yr, y.detach().numpy()) <= 1e-12 and _rel(dr, x.grad.numpy()) <= 1e-12
    assert (ya >= np.abs(yr) * (1 - 1e-12)).all() and (da >= np.abs(dr) * (1 - 1e-12)).all()
    # the fp32-coordinate matrices are the same code: rows sum to one within the rounding of l0 = 1 - l1, same sparsity
    for a32, a64 in zip(rr.bilinear_matrices(*hw, coord='fp32'), rr.bilinear_matrices(*hw, coord='exact')):
        assert a32.dtype == np.float64 and a32.shape == a64.shape
        assert np.abs(a32.sum(axis=1) - 1).max() <= rr.U and np.abs(a32 - a64).max() <= 2.0 ** -23 * max(2 * max(hw), 1)


def test_contributors_and_forms():
    assert rr.contributors(1) == 2 and rr.contributors(3) == 5 and max(rr.contributors(n) for n in range(3, 300)) == 5
    for shape, stream in rr.BIL_CASES:
        n, c, h, w = shape
        assert rr.stream_ok(n, h, w, c) == stream, shape
    # the grids the issue names for (3, 8, 3, 520): forward 2 parts on 36 workgroups, backward 5 parts on 45
    n, c, h, w = rr.BIL_GATHER_SHAPES[0]
    assert (2 * w * (c // 4)) // 1024 == 2 and n * 2 * h * 2 == 36 and (w * (c // 4) + 255) // 256 == 5 and n * h * 5 == 45


def test_nearest_reference():
    for shape in rr.NEAREST_SHAPES:
        x = torch.randn(shape, generator=_gen(3), dtype=torch.float64).requires_grad_(True)
        y = F.interpolate(x, scale_factor=2, mode='nearest')
        dy = torch.randn(y.shape, generator=_gen(4), dtype=torch.float64)
        y.backward(dy)
        assert np.array_equal(rr.nearest_ref(x.detach().numpy()), y.detach().numpy())
        assert _rel(rr.nearest_bwd_ref(dy.numpy()), x.grad.numpy()) <= 1e-15
        # the fp32 (a + b) + (c + d): three roundings at most on sum |.|
        d32 = dy.float().numpy()
        mag = rr.nearest_bwd_ref(np.abs(d32))
        assert rr.worst_ratio(rr.nearest_bwd_f32(d32).astype(np.float64) - rr.nearest_bwd_ref(d32), 2 * rr.U * mag) <= 1.0


@pytest.mark.parametrize('case', rr.AVG_CASES[::3])
def test_avgpool_reference(case):
    o, (h, w), c = case
    x = torch.randn(rr.AVG_N, c, h, w, generator=_gen(5), dtype=torch.float64).requires_grad_(True)
    y = F.adaptive_avg_pool2d(x, (o, o)).view(rr.AVG_N, -1)
    dy = torch.randn(y.shape, generator=_gen(6), dtype=torch.float64)
    y.backward(dy)
    yr, _ = rr.avgpool_ref(x.detach().numpy(), o)
    dr, _ = rr.avgpool_bwd_ref(dy.numpy(), tuple(x.shape), o)
    assert _rel(yr, y.detach().numpy()) <= 1e-14 and _rel(dr, x.grad.numpy()) <= 1e-14


def test_avg_cases_cover_the_cross():
    assert len(rr.AVG_CASES) == 30 and len(set(rr.AVG_CASES)) == 30
    assert {o for o, _, _ in rr.AVG_CASES} == {1, 2, 6, 7} and {c for _, _, c in rr.AVG_CASES} == {1, 3, 8, 20}
    assert {hw for _, hw, _ in rr.AVG_CASES} == {(2, 2), (7, 9), (13, 6), (32, 32), (5, 40)}
    assert any(hw[0] < o for o, hw, _ in rr.AVG_CASES) and any(hw[0] % o for o, hw, _ in rr.AVG_CASES if hw[0] > o)


def test_pixel_gate_and_modulate_references():
    x, psi, dy = rr.gate_inputs((2, 8, 3, 5), 7)
    assert float(psi.abs().max()) <= 10
    xr = x.double().requires_grad_(True); pr = psi.double().requires_grad_(True)
    y = xr * torch.sigmoid(pr)
    y.backward(dy.double())
    ref = rr.pixel_gate_ref(x.numpy(), psi.numpy(), dy.numpy())
    assert _rel(ref['y'], y.detach().numpy()) <= 1e-14 and _rel(ref['dx'], xr.grad.numpy()) <= 1e-14
    assert _rel(ref['dpsi'], pr.grad.numpy()) <= 1e-13 and (ref['mag'] >= np.abs(ref['dpsi']) * (1 - 1e-12)).all()
    x, gb, dy = rr.modulate_inputs((2, 8, 3, 5), 8)
    xr = x.double().requires_grad_(True); gr = gb.double().requires_grad_(True)
    y = xr * (1 + gr[:, :8]) + gr[:, 8:]
    y.backward(dy.double())
    ref = rr.modulate_ref(x.numpy(), gb.numpy(), dy.numpy())
    assert _rel(ref['y'], y.detach().numpy()) <= 1e-14 and _rel(ref['dx'], xr.grad.numpy()) <= 1e-14
    assert _rel(ref['dgam'], gr.grad[:, :8].numpy()) <= 1e-14 and np.array_equal(gr.grad[:, 8:].numpy(), dy.double().numpy())


# ----------------------------------------------------------------------------- the pool's rule, ATen and routing
def test_special_windows_follow_aten_in_both_memory_formats():
    x, expected = rr.special_windows()
    R = len(rr.SPECIAL_PATTERNS)
    assert tuple(x.shape) == (1, 8, 2 * R, 2) and R >= 14
    names = [nm for nm, _ in rr.SPECIAL_PATTERNS]
    for want in ('nan at 0', 'nan at 1', 'nan at 2', 'nan at 3', '[nan, nan, 1, 2]', '[1, nan, 5, nan]', 'all nan', 'all -inf',
                 '[inf, inf, 1, nan]', '[0, -0, 0, -0]', '[-0, 0, -0, 0]', 'all equal', '[1, 5, 5, 2]', '[1, 2, 5, 5]'):
        assert want in names
    for r in range(R):                                      # four different bytes in each channel quad of every window row
        assert sorted(expected[r, :4]) == [0, 1, 2, 3] and sorted(expected[r, 4:]) == [0, 1, 2, 3]
    y, k = rr.maxpool_ref(x)
    assert np.array_equal(k[0, :, 0, :], expected)
    y2, k2 = rr.maxpool_ref(x.contiguous(memory_format=torch.channels_last))
    assert np.array_equal(k2, k) and rr.same_bits(y2, y)
    for r in range(R):
        for c in range(8):
            nm = rr.special_pattern_at(r, c)
            if nm == 'all nan' or nm == '[1, nan, 5, nan]' or nm == '[inf, inf, 1, nan]':
                assert k[0, r, 0, c] == 3 and np.isnan(y[0, c, r, 0])
            if nm == 'all -inf' or nm == '[0, -0, 0, -0]' or nm == '[-0, 0, -0, 0]' or nm == 'all equal':
                assert k[0, r, 0, c] == 0
            if nm == '[-0, 0, -0, 0]':
                assert np.signbit(y[0, c, r, 0])
            if nm == '[0, -0, 0, -0]':
                assert y[0, c, r, 0] == 0 and not np.signbit(y[0, c, r, 0])


@pytest.mark.parametrize('shape', rr.POOL_SHAPES + ['special'])
def test_pool_emulation_and_routing_match_aten(shape):
    x = rr.special_windows()[0] if shape == 'special' else rr.pool_input(shape, 11)
    if shape != 'special' and x.numel() > 100:
        oh_ow = x.numel() // 4
        assert int(torch.isnan(x).sum()) > 0 and oh_ow > 0
    xr = x.clone().requires_grad_(True)
    yr, flat = F.max_pool2d(xr, 2, 2, return_indices=True)
    y, k = rr.maxpool_ref(x)
    ye, ke = rr.maxpool_emul(x.numpy())
    assert rr.same_bits(ye, y) and np.array_equal(ke, k)
    dy = torch.randn(yr.shape, generator=_gen(12))
    z = torch.randn(yr.shape, generator=_gen(13)).requires_grad_(True)
    u = F.max_unpool2d(z, flat, 2, 2)
    du = torch.randn(u.shape, generator=_gen(14))
    yr.backward(dy); u.backward(du)
    assert rr.same_bits(rr.scatter_ref(dy.numpy(), k), xr.grad.numpy())
    assert rr.same_bits(rr.scatter_ref(z.detach().numpy(), k), u.detach().numpy())
    assert rr.same_bits(rr.gather_ref(du.numpy(), k), z.grad.numpy())


@pytest.mark.parametrize('defect', ['first_nan', 'last_tie', 'swap_bytes'])
@pytest.mark.parametrize('shape', [(3, 20, 38, 50), 'special'])
def test_pool_defects_are_seen(shape, defect):
    x = rr.special_windows()[0] if shape == 'special' else rr.pool_input(shape, 11)
    y, k = rr.maxpool_ref(x)
    yd, kd = rr.maxpool_emul(x.numpy(), **{defect: True})
    assert not np.array_equal(kd, k)                                        # idx, byte for byte
    dy = torch.randn(y.shape, generator=_gen(12)).numpy()
    du = torch.randn(x.shape, generator=_gen(14)).numpy()
    assert not rr.same_bits(rr.scatter_ref(dy, kd), rr.scatter_ref(dy, k))  # pool backward / unpool forward
    assert not rr.same_bits(rr.gather_ref(du, kd), rr.gather_ref(du, k))    # unpool backward
    if defect == 'swap_bytes':
        assert rr.same_bits(yd, y)                                          # the pooled values alone would not have seen it
    if defect == 'last_tie' and shape == 'special':
        assert not rr.same_bits(yd, y)                                      # [0, -0, 0, -0]: the sign of the zero


# ----------------------------------------------------------------------------- emulations through the gates, every shape
def _bil_inputs(shape, seed=21):
    n, c, h, w = shape
    g = _gen(seed)
    return torch.randn(shape, generator=g).numpy(), torch.randn(n, c, 2 * h, 2 * w, generator=g).numpy()


@pytest.mark.parametrize('shape,stream', rr.BIL_CASES)
def test_bilinear_emulation_passes_its_gates(shape, stream):
    x, dy = _bil_inputs(shape)
    r = rr.bilinear_ratios(x, dy, rr.bilinear_fwd_emul(x), rr.bilinear_bwd_emul(dy, stream), stream)
    _report('bilinear %s' % ('stream' if stream else 'gather'), r)
    assert r['fwd'] <= 1.0 and r['bwd'] <= 1.0, (shape, r)
    if stream and shape[2] * shape[3] <= 2048:
        # "the results agree to the last bit except where x0 == x1": the two backward forms differ in the last column at most
        a, b = rr.bilinear_bwd_emul(dy, True), rr.bilinear_bwd_emul(dy, False)
        assert rr.same_bits(a[..., :-1], b[..., :-1])


@pytest.mark.parametrize('shape', [(2, 16, 141, 3), (2, 16, 70, 9), (2, 64, 128, 128)])
def test_unrounded_coordinate_fails_the_forward_gate(shape):
    x, dy = _bil_inputs(shape)
    yr, ya = rr.bilinear_ref(x)
    r = rr.worst_ratio(rr.bilinear_fwd_emul(x, unrounded=True).astype(np.float64) - yr, rr.bil_gate(rr.K_BIL_FWD, ya))
    print('unrounded coordinate %s: error / gate %.1f' % (shape, r))
    assert r > 1.0


@pytest.mark.parametrize('shape,stream', [((1, 4, 2, 1100), False), ((2, 8, 5, 7), False), ((3, 8, 3, 520), False),
                                          ((2, 16, 17, 65), True), ((2, 16, 3, 3), True), ((2, 64, 128, 128), True)])
def test_dropped_fifth_column_fails_the_backward_gate(shape, stream):
    x, dy = _bil_inputs(shape)
    r = rr.bilinear_ratios(x, dy, rr.bilinear_fwd_emul(x), rr.bilinear_bwd_emul(dy, stream, drop_fifth=True), stream)
    print('dropped fifth column %s: error / gate %.1f' % (shape, r['bwd']))
    assert r['bwd'] > 1.0 and r['fwd'] <= 1.0


@pytest.mark.parametrize('shape', [(2, 16, 17, 65), (2, 32, 70, 9), (2, 80, 141, 3), (2, 64, 128, 128)])
def test_dropped_band_boundary_row_fails_the_backward_gate(shape):
    x, dy = _bil_inputs(shape)
    r = rr.bilinear_ratios(x, dy, rr.bilinear_fwd_emul(x), rr.bilinear_bwd_emul(dy, True, drop_band_row=True), True)
    print('dropped band row %s: error / gate %.1f' % (shape, r['bwd']))
    assert r['bwd'] > 1.0


def _avg_inputs(case, seed=31):
    o, (h, w), c = case
    g = _gen(seed)
    return torch.randn(rr.AVG_N, c, h, w, generator=g).numpy(), torch.randn(rr.AVG_N, c * o * o, generator=g).numpy()


@pytest.mark.parametrize('case', rr.AVG_CASES)
def test_avgpool_emulation_passes_its_gates(case):
    x, dy = _avg_inputs(case)
    r = rr.avgpool_ratios(x, case[0], dy, rr.avgpool_emul(x, case[0]), rr.avgpool_bwd_emul(dy, x.shape, case[0]))
    _report('avgpool', r)
    assert r['fwd'] <= 1.0 and r['bwd'] <= 1.0, (case, r)


@pytest.mark.parametrize('case', [c for c in rr.AVG_CASES if c[1][0] % c[0] or c[1][1] % c[0]])
def test_floored_bin_end_fails_the_avgpool_gates(case):
    x, dy = _avg_inputs(case)
    o = case[0]
    r = rr.avgpool_ratios(x, o, dy, rr.avgpool_emul(x, o, floor_hi=True), rr.avgpool_bwd_emul(dy, x.shape, o, floor_hi=True))
    assert r['fwd'] > 1.0 and r['bwd'] > 1.0, (case, r)


@pytest.mark.parametrize('shape', rr.GATE_CASES)
def test_pixel_gate_emulation_passes_its_gates(shape):
    x, psi, dy = (t.numpy() for t in rr.gate_inputs(shape, 41))
    r = rr.pixel_gate_ratios(x, psi, dy, rr.pixel_gate_emul(x, psi, dy))
    _report('pixel gate', r)
    assert max(r.values()) <= 1.0, (shape, r)


@pytest.mark.parametrize('shape', [s for s in rr.GATE_CASES if s[1] > 64])
def test_single_pass_channel_loop_fails_the_pixel_gate_gates(shape):
    x, psi, dy = (t.numpy() for t in rr.gate_inputs(shape, 41))
    r = rr.pixel_gate_ratios(x, psi, dy, rr.pixel_gate_emul(x, psi, dy, first_pass_only=True))
    assert r['dpsi'] > 1.0 and r['dx'] > 1.0 and r['y'] <= 1.0, (shape, r)


@pytest.mark.parametrize('shape', rr.MOD_CASES)
def test_modulate_emulation_passes_and_shifted_beta_fails(shape):
    x, gb, dy = (t.numpy() for t in rr.modulate_inputs(shape, 51))
    r = rr.modulate_ratios(x, gb, dy, rr.modulate_emul(x, gb, dy))
    _report('modulate', r)
    assert max(r.values()) <= 1.0, (shape, r)
    bad = rr.modulate_ratios(x, gb, dy, rr.modulate_emul(x, gb, dy, beta_offset=shape[1] - 4))
    assert bad['y'] > 1.0


def test_nearest_emulation_is_its_own_reference():
    for shape in rr.NEAREST_SHAPES:
        dy = torch.randn(shape[0], shape[1], 2 * shape[2], 2 * shape[3], generator=_gen(61)).numpy()
        a = rr.nearest_bwd_f32(dy)
        b = (dy[:, :, 0::2, 0::2] + dy[:, :, 1::2, 0::2]) + (dy[:, :, 0::2, 1::2] + dy[:, :, 1::2, 1::2])    # another grouping
        assert a.shape == tuple(shape) and not rr.same_bits(a, b) or a.size < 64
