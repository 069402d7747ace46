"""CPU rehearsal of the gates tests/test_conv_s2_bf16x1_gpu.py sets (tests/s2_bf16x1_ref.py): the parity-class decomposition is
the gradient of the stride-2 conv, the a-priori bound holds on the test shapes, a STAND-IN for the kernels -- the same rounded
operands convolved with fp32 accumulation on the CPU -- passes gates (b) and (c) at every case (so the gates are ones the
reference alone stays within), and a dropped tap or a class written at the wrong offset fails them."""
import pytest
import torch
import torch.nn.functional as F

import s2_bf16x1_ref as R


@pytest.mark.parametrize('h,w', [(18, 34), (21, 71), (16, 37), (7, 8)])
def test_parity_classes_are_the_autograd_gradient(h, w):
    """Even and odd sizes: four classes with 1, 2, 2, 4 taps at offsets {0, +1} assemble the fp64 gradient of
    F.conv2d(stride=2, padding=1)."""
    g = torch.Generator().manual_seed(h * 100 + w)
    oh, ow = R.out_hw(h, w)
    dy = torch.randn(2, 5, oh, ow, generator=g, dtype=torch.float64)
    wt = torch.randn(5, 6, 3, 3, generator=g, dtype=torch.float64)
    cls = R.classes()
    assert [len(t) for _, _, t in cls] == [1, 2, 2, 4]
    assert all(oy in (0, 1) and ox in (0, 1) for _, _, taps in cls for _, _, oy, ox in taps)
    want = R.dgrad64(dy, wt, h, w)
    assert want.abs().max() > 1
    got = R.dgrad_by_classes(dy, wt, h, w)
    assert (got - want).abs().max().item() <= 1e-12
    assert (R.dgrad_by_classes(dy, wt, h, w, 2, 5) - want[:, 2:5]).abs().max().item() <= 1e-12
    # the deliberate faults are faults
    assert (R.dgrad_by_classes(dy, wt, h, w, drop_tap=(3, 2)) - want).abs().max().item() > 0.1
    assert (R.dgrad_by_classes(dy, wt, h, w, shift_class=1) - want).abs().max().item() > 0.1


@pytest.mark.parametrize('name', sorted(R.FWD_CASES))
def test_forward_standin_passes_the_gates(name):
    n, ci, co, h, w = R.FWD_CASES[name]
    x, wt = R.make_fwd_case(name)
    bias = torch.randn(co, generator=torch.Generator().manual_seed(9))
    bound = R.conv_bound(x, wt)
    err = (R.conv_ref(x, wt) - R.conv64(x, wt)).abs()
    print('%s: worst |conv_ref - fp64| / apriori_bound = %.3f' % (name, (err / bound).max().item()))
    assert (err <= bound).all()
    for act, slope in ((None, 0.0), ('lrelu', 0.2)):
        y = R._act(F.conv2d(R.rb(x), R.rb(wt), bias, 2, 1), act, slope).double()
        ref, exact = R.conv_ref(x, wt, bias, act, slope), R.conv64(x, wt, bias, act, slope)
        b_ok, c_ok, fig = R.gates(y, y, ref, exact, bound)
        assert b_ok and c_ok, fig
        # a dropped tap (the corner tap's weights zeroed in the stand-in only) fails both
        wbad = R.rb(wt).clone(); wbad[:, :, 2, 2] = 0
        ybad = R._act(F.conv2d(R.rb(x), wbad, bias, 2, 1), act, slope).double()
        b_ok, c_ok, _ = R.gates(ybad, y, ref, exact, bound)
        assert not b_ok and not c_ok


@pytest.mark.parametrize('name', sorted(R.DGRAD_CASES))
def test_input_gradient_standin_passes_the_gates(name):
    n, o, i, c_lo, c_hi, h, w = R.DGRAD_CASES[name]
    dy, wt = R.make_dgrad_case(name)
    bound = R.dgrad_bound(dy, wt, h, w, c_lo, c_hi)
    ref, exact = R.dgrad_ref(dy, wt, h, w, c_lo, c_hi), R.dgrad64(dy, wt, h, w, c_lo, c_hi)
    assert ((ref - exact).abs() <= bound).all()
    y = R.dgrad_by_classes(R.rb(dy), R.rb(wt), h, w, c_lo, c_hi, dtype=torch.float32).double()
    b_ok, c_ok, fig = R.gates(y, y, ref, exact, bound)
    assert b_ok and c_ok, fig
    for fault in (dict(drop_tap=(3, 1)), dict(drop_tap=(0, 0)), dict(shift_class=2)):
        ybad = R.dgrad_by_classes(R.rb(dy), R.rb(wt), h, w, c_lo, c_hi, dtype=torch.float32, **fault).double()
        b_ok, c_ok, _ = R.gates(ybad, y, ref, exact, bound)
        assert not b_ok and not c_ok, fault
