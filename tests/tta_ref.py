"""The definitions of flip / rotation test-time augmentation restated in numpy and, for the GPU tests, in torch:
the eight views T_k of a square array, their inverses, the balanced-tree mean, and the index maps the kernels of csrc/sw_tta.hip
use in place of moving data.  A view is a D4 code k in 0 .. 7 with f = k >> 2, r = k & 3."""
import numpy as np

SETS = {'hflip': (0, 4), 'flips': (0, 4, 2, 6), 'd4': (0, 1, 2, 3, 4, 5, 6, 7)}


def T(a, k):
    """T_k(a) = rot90(fliplr(a) if f else a, r) on the first two axes; np.rot90 is counter-clockwise."""
    f, r = k >> 2, k & 3
    return np.rot90(np.fliplr(a) if f else a, r)


def T_inv(y, k):
    """T_k^-1(y) = fliplr(u) if f else u, u = rot90(y, 4 - r)."""
    f, r = k >> 2, k & 3
    u = np.rot90(y, 4 - r)
    return np.fliplr(u) if f else u


def tree_mean(qs):
    """Balanced tree in list order, fp32, times 1 / K; K = 1: the array itself."""
    qs = [np.asarray(q, dtype=np.float32) for q in qs]
    k = len(qs)
    assert k in (1, 2, 4, 8)
    if k == 1:
        return qs[0]
    while len(qs) > 1:
        qs = [qs[i] + qs[i + 1] for i in range(0, len(qs), 2)]
    return qs[0] * np.float32(1.0 / k)


def index_map(k, inverse):
    """(swap, rev_y, rev_x) of csrc/sw_tta.hip's sw_d4_map: pixel (i, j) of T_k(a) (inverse false) or of T_k^-1(a) (inverse true)
    is a[rev_y(p), rev_x(q)], (p, q) = (j, i) if swap else (i, j), rev(t) = S - 1 - t or t."""
    f, r = k >> 2, k & 3
    if r == 0:
        return (False, False, bool(f))
    if r == 2:
        return (False, True, not f)
    if not inverse:
        return (True, r == 3, (r == 1) != bool(f))
    return (True, (r == 1) != bool(f), r == 3)


def apply_index_map(a, m):
    """The array the kernels produce from `a` under the map m, pixel by pixel."""
    swap, rev_y, rev_x = m
    s = a.shape[0]
    out = np.empty_like(a)
    for i in range(s):
        for j in range(s):
            p, q = (j, i) if swap else (i, j)
            out[i, j] = a[s - 1 - p if rev_y else p, s - 1 - q if rev_x else q]
    return out


# ----------------------------------------------------------------------------- torch, on the H, W axes of [N, C, H, W]
def T_t(x, k):
    import torch
    f, r = k >> 2, k & 3
    return torch.rot90(torch.flip(x, (3,)) if f else x, r, (2, 3))


def T_inv_t(y, k):
    import torch
    f, r = k >> 2, k & 3
    u = torch.rot90(y, 4 - r, (2, 3))
    return torch.flip(u, (3,)) if f else u


def tree_mean_t(qs):
    qs = list(qs)
    k = len(qs)
    assert k in (1, 2, 4, 8)
    if k == 1:
        return qs[0].clone()
    while len(qs) > 1:
        qs = [qs[i] + qs[i + 1] for i in range(0, len(qs), 2)]
    return qs[0] * (1.0 / k)
