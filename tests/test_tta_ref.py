"""CPU: the definitions of test-time augmentation (tests/tta_ref.py) against numpy itself -- inverses, the named sets, the
commutation the oriented gather kernel relies on, the exactness of the tree mean, and the kernels' index maps."""
import numpy as np
import pytest

import tta_ref as R


def _asym(s):
    return np.arange(s * s, dtype=np.float32).reshape(s, s) * 1.5 + 0.25


@pytest.mark.parametrize('s', [5, 1])
@pytest.mark.parametrize('k', range(8))
def test_inverse_undoes_the_view(s, k):
    a = _asym(s)
    assert np.array_equal(R.T_inv(R.T(a, k), k), a)
    assert np.array_equal(R.T(R.T_inv(a, k), k), a)
    if s > 1 and k:
        assert not np.array_equal(R.T(a, k), a)                             # the array has no symmetry to hide behind


def test_the_eight_views_are_distinct_and_the_named_sets_are_what_they_say(pkg):
    a = _asym(5)
    assert len({R.T(a, k).tobytes() for k in range(8)}) == 8
    assert np.array_equal(R.T(a, 0), a)
    assert np.array_equal(R.T(a, 4), np.fliplr(a))
    assert np.array_equal(R.T(a, 2), np.rot90(a, 2)) and np.array_equal(R.T(a, 2), a[::-1, ::-1])
    assert np.array_equal(R.T(a, 6), np.flipud(a))
    assert np.array_equal(R.T(a, 1), np.rot90(a)) and R.T(a, 1)[1, 3] == a[3, 5 - 1 - 1]
    assert np.array_equal(R.T(a, 5), a.T) and np.array_equal(R.T(a, 7), a.T[::-1, ::-1])   # fliplr, then 90: the transpose
    assert R.SETS == {'hflip': (0, 4), 'flips': (0, 4, 2, 6), 'd4': tuple(range(8))}
    assert pkg.ops.TTA_SETS == R.SETS


@pytest.mark.parametrize('factor', [1, 2])
def test_box_resize_commutes_with_every_view(pkg, factor):
    """(a + b + c + d + 2) >> 2 is symmetric in its four bytes: orienting the resized patch and resizing the oriented patch are
    the same bytes, which is why the gather kernel may fold the view into its index map."""
    A = pkg.aerial_image_segmentation_api
    rng = np.random.default_rng(60)
    for size in (1, 3, 8):
        patch = rng.integers(0, 256, (size * factor, size * factor, 3), dtype=np.uint8)
        for k in range(8):
            a = R.T(A.resize_u8(patch, size, size), k)
            b = A.resize_u8(np.ascontiguousarray(R.T(patch, k)), size, size)
            assert np.array_equal(a, b), (size, k)
            # and the per-pixel normalisation follows
            assert np.array_equal(R.T(A.normalize_imagenet(A.resize_u8(patch, size, size)), k), A.normalize_imagenet(b))


@pytest.mark.parametrize('k', [2, 4, 8])
def test_tree_mean_of_equal_arrays_is_the_array(k):
    rng = np.random.default_rng(61)
    q = rng.random((3, 7, 7), dtype=np.float32)
    q[0, 0, :4] = (0.0, 1.0, np.float32(1e-38), np.nextafter(np.float32(1), np.float32(0)))
    got = R.tree_mean([q] * k)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), q.view(np.int32))


def test_tree_mean_is_the_tree_of_the_definition():
    rng = np.random.default_rng(62)
    q = [rng.random((4, 4), dtype=np.float32) for _ in range(8)]
    f = np.float32
    assert np.array_equal(R.tree_mean(q[:1]), q[0])
    assert np.array_equal(R.tree_mean(q[:2]), (q[0] + q[1]) * f(0.5))
    assert np.array_equal(R.tree_mean(q[:4]), ((q[0] + q[1]) + (q[2] + q[3])) * f(0.25))
    assert np.array_equal(R.tree_mean(q), (((q[0] + q[1]) + (q[2] + q[3])) + ((q[4] + q[5]) + (q[6] + q[7]))) * f(0.125))
    left = ((((((q[0] + q[1]) + q[2]) + q[3]) + q[4]) + q[5]) + q[6]) + q[7]
    assert not np.array_equal(R.tree_mean(q), left * f(0.125))              # the order is part of the definition


@pytest.mark.parametrize('s', [5, 1, 4])
@pytest.mark.parametrize('k', range(8))
def test_index_maps_of_the_kernels_are_the_views(s, k):
    a = _asym(s)
    assert np.array_equal(R.apply_index_map(a, R.index_map(k, False)), R.T(a, k))
    assert np.array_equal(R.apply_index_map(a, R.index_map(k, True)), R.T_inv(a, k))
    assert R.index_map(k, False)[0] == R.index_map(k, True)[0] == bool(k & 1)   # the odd rotations are the transposing ones
