"""CPU: which body a launch of the split LDS-DMA conv family (kernel ids 50 / 51: 1x1, stride-2 3x3, parity classes) runs.

ssg_conv_dma_body (a diagnostic export outside include/ssunet_hip.h) reports 2 for the split-once body of
csrc/conv_igemm_dma_k32.hip and 1 where that body does not run: conv_igemm_dma_x3_kernel for a descriptor its predicate
(ssg_conv_dma_k32_ok) declines, the fp32 LDS-DMA kernel for a descriptor without a split pack (what ops.py sends under
SSG_MFMA_SPLIT=0); 0 for a descriptor of another family.  Descriptors are the dummy aligned ones of tests/test_conv_plan.py;
nothing is launched or dereferenced."""
import ctypes

import pytest

from test_conv_plan import BIAS, PART, RES, ROWS, WSPLIT, _conv_desc, _opt

FAMILY = [spec for spec, want in ROWS if spec[0] != 'wgrad' and want[0].startswith('conv_igemm_dma_x3_kernel')]
STEP = [s for s in FAMILY if not _opt(s[-1], 'mis')]


def _body(pkg, d):
    fn = pkg._lib.load().ssg_conv_dma_body
    fn.argtypes = [ctypes.POINTER(pkg._lib.ConvDesc)]
    fn.restype = ctypes.c_int
    return fn(ctypes.byref(d)) if d is not None else fn(None)


def _split_desc(pkg, spec):
    """The descriptor of tests/test_conv_plan.py::conv_row at the point of the launch: split pack and statistics rows attached."""
    d = _conv_desc(pkg._lib, spec)
    if not _opt(spec[-1], 'fp32'):
        assert pkg._lib.call('ssg_conv2d_split_bn', ctypes.byref(d)) in (64, 128)
        d.w_split = WSPLIT
    if _opt(spec[-1], 'bn'):
        d.bnpart = PART
    return d


def test_the_family_rows_are_there():
    assert len(STEP) >= 20 and any(s[7] == 3 and s[8] == 2 for s in STEP) and any(s[3] for s in STEP) and any('class' in s[-1] for s in STEP)


@pytest.mark.parametrize('spec', STEP, ids=['%s n%d c%d+%d %dx%d o%d k%d s%d %s' % s[:10] for s in STEP])
def test_step_rows_run_the_split_once_body(pkg, spec):
    d = _split_desc(pkg, spec)
    assert pkg._lib.call('ssg_conv2d_kernel_id', ctypes.byref(d)) in (50, 51)
    assert _body(pkg, d) == 2


BASE = ('fwd', 16, 128, 0, 256, 256, 128, 1, 1, 'bias res relu')


def _edge(pkg, name):
    d = _split_desc(pkg, BASE)
    if name == 'out 4 bytes off 16':
        d.out = d.out + 4
    elif name == 'ldo not a quad':
        d.ldo = d.ldo + 1
    elif name == 'res 4 bytes off 16':
        d.res = RES + 4
    elif name == 'ldr not a quad':
        d.ldr = d.ldr + 1
    elif name == 'bias 4 bytes off 16':
        d.bias = BIAS + 4
    elif name == 'w_split 8 bytes off 16':               # ssg_conv2d_f32 refuses this descriptor (SSG_EALIGN) before a body is chosen
        d.w_split = WSPLIT + 8
    elif name == 'split pack beyond 31-bit byte offsets':  # 16384 x 32768 weights: Cout * Kp * 6 B = 3.2 GB
        d = _split_desc(pkg, ('fwd', 1, 32768, 0, 64, 64, 16384, 1, 1, ''))
    elif name == 'mis row of the plan test':
        d = _split_desc(pkg, ('fwd', 16, 128, 0, 256, 256, 128, 1, 1, 'mis'))
    else:
        assert name == 'none'
    return d


@pytest.mark.parametrize('name', ['out 4 bytes off 16', 'ldo not a quad', 'res 4 bytes off 16', 'ldr not a quad', 'bias 4 bytes off 16',
                                  'w_split 8 bytes off 16', 'split pack beyond 31-bit byte offsets', 'mis row of the plan test'])
def test_edges_the_predicate_excludes_keep_the_old_body(pkg, name):
    assert _body(pkg, _edge(pkg, 'none')) == 2
    d = _edge(pkg, name)
    assert pkg._lib.call('ssg_conv2d_kernel_id', ctypes.byref(d)) in (50, 51)        # the plan does not move: same id, same label
    assert _body(pkg, d) == 1


@pytest.mark.parametrize('spec', [s[:-1] + ((s[-1] + ' fp32').strip(),) for s in STEP[:6]] + [('dgrad', 16, 64, 0, 512, 512, 64, 3, 2, 'class=0 fp32')],
                         ids=lambda s: '%s c%d o%d k%d s%d' % (s[0], s[2], s[6], s[7], s[8]))
def test_fp32_mode_never_runs_it(pkg, spec):
    d = _split_desc(pkg, spec)                            # no split pack: SSG_MFMA_SPLIT=0
    assert not d.w_split
    assert pkg._lib.call('ssg_conv2d_kernel_id', ctypes.byref(d)) in (20, 21, 22)
    assert _body(pkg, d) == 1


def test_other_families_and_bad_descriptors_report_zero(pkg):
    assert _body(pkg, None) == 0
    for spec in (('fwd', 16, 128, 0, 256, 256, 128, 3, 1, 'bn'), ('fwd', 16, 64, 0, 512, 512, 3, 1, 1, ''), ('fwd', 16, 64, 0, 512, 512, 128, 1, 1, '')):
        d = _conv_desc(pkg._lib, spec)
        if pkg._lib.call('ssg_conv2d_split_bn', ctypes.byref(d)):
            d.w_split = WSPLIT
        assert _body(pkg, d) == 0, spec
    d = _split_desc(pkg, BASE)
    d.ntaps = 0
    assert _body(pkg, d) == 0
