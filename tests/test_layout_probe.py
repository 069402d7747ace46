"""Self-test of tests/layout_probe.py on CPU tensors with plain torch writes: each violation of the NHWC memory contract
that tests/test_layout_contract_gpu.py looks for is planted in turn and must be reported; a clean write must pass.  This is
the proof, without a GPU, that the GPU test fails when a kernel is wrong."""
import pytest
import torch

import layout_probe as lp


def _alloc_and_write(alloc, c=3, zero=False):
    t = alloc(2, c, 5, 7, 'cpu', zero=zero)
    if not zero:
        rec = alloc.records[-1]
        p = rec.payload()
        p[:, :c] = torch.randn(p.shape[0], c)
        p[:, c:lp.pad4(c)] = 0.0
    return t, alloc.records[-1]


def test_guarded_allocator_returns_what_new_nhwc_returns(pkg):
    alloc = lp.GuardedAllocator()
    for c, ld, zero in ((3, None, False), (8, None, True), (4, 12, False), (1, None, False)):
        want = pkg.ops.new_nhwc(2, c, 5, 7, 'cpu', ld=ld, zero=zero)
        got = alloc(2, c, 5, 7, 'cpu', ld=ld, zero=zero)
        assert got.shape == want.shape and got.stride() == want.stride() and got.dtype == want.dtype
        assert not got._is_view() and got.data_ptr() % 16 == 0
        assert pkg.ops.nhwc_ld(got) == pkg.ops.nhwc_ld(want)
        ldv = want.stride(3)
        # the storage covers the trailing pad lanes and the back guard
        assert got.untyped_storage().nbytes() // 4 >= got.storage_offset() + 2 * 5 * 7 * ldv + alloc.guard
        if zero:
            assert int(got.abs().sum()) == 0
        else:
            assert bool(lp.is_canary(got).all())
    assert alloc.records[0].who == 'test_guarded_allocator_returns_what_new_nhwc_returns'
    assert len(alloc.records) == 4


def test_install_patches_both_names_and_restores_them(pkg):
    real = pkg.ops.new_nhwc
    assert pkg.blocks.new_nhwc is real
    with pytest.MonkeyPatch.context() as mp:
        alloc = lp.GuardedAllocator().install(mp, pkg)
        assert pkg.ops.new_nhwc is alloc and pkg.blocks.new_nhwc is alloc
    assert pkg.ops.new_nhwc is real and pkg.blocks.new_nhwc is real


def test_clean_write_passes_and_empty_record_fails():
    alloc = lp.GuardedAllocator()
    with pytest.raises(AssertionError, match='saw no allocation'):
        alloc.check()
    _alloc_and_write(alloc, c=3)
    _alloc_and_write(alloc, c=8)
    _alloc_and_write(alloc, c=5, zero=True)         # zero=True: nothing has to be written
    alloc.check()
    assert len(alloc.records) == 3


def test_nonzero_pad_lane_is_reported():
    alloc = lp.GuardedAllocator()
    _, rec = _alloc_and_write(alloc, c=3)
    alloc.check()
    rec.payload()[(1 * 5 + 2) * 7 + 4, 3] = 1e-30
    with pytest.raises(AssertionError) as e:
        alloc.check()
    msg = str(e.value)
    assert '1 pad-lane elements are not zero' in msg and '(1, 2, 4, 3)' in msg
    assert 'new_nhwc(2, 3, 5, 7, ld=4)' in msg and '_alloc_and_write()' in msg
    # a pad lane that was never written (still the canary) is a violation too, also under zero=False
    rec.payload()[:, 3] = 0.0
    alloc.check()
    lp.canary_fill_(rec.payload()[0:1, 3])
    with pytest.raises(AssertionError, match='pad-lane'):
        alloc.check()
    # any NaN fails `== 0`; -0.0 is a zero (what 0 * -w leaves behind)
    rec.payload()[:, 3] = 0.0
    rec.payload()[5, 3] = float('nan')
    with pytest.raises(AssertionError, match='pad-lane'):
        alloc.check()
    rec.payload()[5, 3] = -0.0
    alloc.check()


def test_unwritten_element_is_reported():
    alloc = lp.GuardedAllocator()
    _, rec = _alloc_and_write(alloc, c=6)
    alloc.check()
    lp.canary_fill_(rec.payload()[(0 * 5 + 4) * 7 + 6:(0 * 5 + 4) * 7 + 7, 5])
    with pytest.raises(AssertionError) as e:
        alloc.check()
    assert '1 elements of real channel lanes never written' in str(e.value) and '(0, 4, 6, 5)' in str(e.value)


def test_front_guard_write_is_reported():
    alloc = lp.GuardedAllocator()
    _, rec = _alloc_and_write(alloc, c=4)
    rec.buf[rec.guard - 1] = 0.0
    with pytest.raises(AssertionError) as e:
        alloc.check()
    assert 'front guard overwritten, 1 floats, first 1 floats before' in str(e.value)


def test_back_guard_write_is_reported():
    alloc = lp.GuardedAllocator()
    _, rec = _alloc_and_write(alloc, c=4)
    rec.buf[rec.guard + 2 * 5 * 7 * 4 + 2] = float('nan')         # another NaN is not the canary
    with pytest.raises(AssertionError) as e:
        alloc.check()
    assert 'back guard overwritten, 1 floats, first 2 floats past' in str(e.value)


def test_poisoned_slice_layout_and_neighbour_detection(pkg):
    x = torch.randn(2, 8, 3, 5)
    for ld, c0 in ((12, 0), (16, 0), (12, 4), (16, 8)):
        v = lp.poisoned_slice(x, ld, c0, 'cpu')
        assert pkg.ops.nhwc_ld(v) == ld and not v._is_view()
        assert torch.equal(v, x)
        lp.check_slice(v)
        rec = v._layout_probe
        p = rec.buf[rec.guard:rec.guard + 2 * 3 * 5 * ld].view(-1, ld)
        assert int(lp.is_canary(p).sum()) == 2 * 3 * 5 * (ld - 8)
        lane = c0 + 8 if c0 + 8 < ld else c0 - 1
        p[(1 * 3 + 2) * 5 + 3, lane] = 0.0                          # what an in-place op over whole pixel rows would do
        with pytest.raises(AssertionError) as e:
            lp.check_slice(v)
        assert '1 elements of neighbouring lanes overwritten' in str(e.value) and '(1, 2, 3, %d)' % lane in str(e.value)
    for bad in ((6, 8, 0), (8, 12, 2), (8, 12, 8)):
        with pytest.raises(ValueError):
            lp.poisoned_slice(torch.randn(1, bad[0], 2, 2), bad[1], bad[2], 'cpu')


def test_destination_slice_must_be_written_and_guards_hold():
    d = lp.canary_slice(1, 4, 3, 3, 8, 4, 'cpu')
    with pytest.raises(AssertionError, match='36 elements of the slice never written'):
        lp.check_slice(d, written=True)
    d.copy_(torch.randn(1, 4, 3, 3))
    lp.check_slice(d, written=True)
    rec = d._layout_probe
    rec.buf[rec.guard + 1 * 3 * 3 * 8] = 1.0
    with pytest.raises(AssertionError, match='back guard overwritten'):
        lp.check_slice(d, written=True)
    rec.buf[0] = 1.0
    with pytest.raises(AssertionError, match='front guard overwritten'):
        lp.check_slice(d)
