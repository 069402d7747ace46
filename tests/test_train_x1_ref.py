"""CPU rehearsal of the block gate of tests/test_train_x1_gpu.py.  train_x1_ref.stats gives, per gradient and for the output, the
(max, RMS) error of the quantised fp64 BasicBlock against the unquantised one at the GPU test's shapes and seeds, both under the
same imposed ReLU masks; the device's error may be at most 1.5 x (max) / 1.25 x (RMS) of that.

What the gate can see.  A routing mistake is a LAUNCH on the wrong kernel: both rounding sites of one of the six routed launches
missing, or the 1x1 shortcut rounded.  Each is shown to move the RMS statistic of at least one tensor outside the 1.25 margin
(below 1 / 1.25 for a missing launch -- the two sites of a launch contribute equally and independently, so the tensor the launch
produces drops to ~1 / sqrt(2) = 0.71 -- above it for the shortcut: wsc goes from exactly zero to 2^-9-sized errors).  ONE site
of a launch alone is NOT outside the margin, and cannot be: it removes a quarter of the variance of the tensor its launch
produces, sqrt(3/4) = 0.87 > 0.8.  The measured single-site ratios are printed and asserted to lie in (0.8, 1) for the tensor
the launch produces; the device gate is one-sided, so a missing launch on the GPU is what the routing test's kernel ids catch."""
import pytest

import train_x1_ref as tr

MODES = ('train', 'frozen')
# the tensor each routed launch produces
PRODUCES = {'f1': None, 'f2': 'out', 'd2': 'b1', 'd1': 'x1', 'w2': 'w2', 'w1': 'w1'}


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case', sorted(tr.CASES))
def test_reference_statistics(case, mode):
    st = tr.stats(case, mode)
    n, c1, c2, planes, h, w = tr.CASES[case]
    want = {'out', 'x1', 'w1', 'w2', 'g1', 'b1', 'g2', 'b2'} | ({'x2', 'wsc'} if c2 else set())
    assert set(st) == want
    for k, (mx, rms, scale) in st.items():
        print('STAT %-7s %-6s %-3s max %.3e rms %.3e   (max|T| %.3e)' % (case, mode, k, mx, rms, scale))
        if k in ('wsc', 'b2'):
            assert mx == 0        # no rounding site reaches the shortcut's weight gradient or the sum of the masked dout
        else:
            # bf16 rounding moves every other tensor, by a small fraction of its size
            assert 0 < rms <= mx < 0.1 * scale, (k, mx, rms, scale)


def _ratios(case, mode, sites):
    ref = tr.stats(case, mode)
    got = tr.stats(case, mode, sites)
    return {k: (got[k][1] / ref[k][1] if ref[k][1] else (float('inf') if got[k][1] else 1.0)) for k in ref}


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('launch', sorted(tr.LAUNCHES))
def test_a_launch_left_unrounded_moves_a_statistic_outside_the_margin(launch, mode):
    r = _ratios('cat128', mode, tr.ALL - set(tr.LAUNCHES[launch]))
    out = {k: round(v, 3) for k, v in r.items() if v < 1 / tr.RMS_MARGIN or v > tr.RMS_MARGIN}
    print(launch, mode, out)
    assert out, 'no statistic sees launch %s on the fp32-class kernel: %s' % (launch, r)
    if PRODUCES[launch]:
        assert r[PRODUCES[launch]] < 1 / tr.RMS_MARGIN


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('site', sorted(tr.ALL))
def test_one_site_alone_stays_inside_the_margin(site, mode):
    """The figures behind the module docstring: one site removes about a quarter of the variance of its launch's tensor."""
    r = _ratios('cat128', mode, tr.ALL - {site})
    k = PRODUCES[site[:2]]
    print(site, mode, {a: round(b, 3) for a, b in r.items()})
    assert all(v < tr.RMS_MARGIN for v in r.values())          # fewer roundings never fail the (one-sided) device gate
    if k and not (k == 'b1' and site.startswith('d2')):      # b1 is a column sum: its two sites do not weigh equally
        assert 1 / tr.RMS_MARGIN < r[k] < 1, (site, k, r[k])


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('sites', [('scdy',), ('scx', 'scw', 'scdy')], ids=['scdy', 'shortcut_routed'])
def test_a_rounding_added_at_the_shortcut_fails_the_gate(sites, mode):
    r = _ratios('cat128', mode, tr.ALL | set(sites))
    print(sites, mode, {a: round(b, 3) for a, b in r.items()})
    assert r['wsc'] > tr.RMS_MARGIN
