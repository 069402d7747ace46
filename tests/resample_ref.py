"""Plain references for the memory-bound kernels between the convolutions: csrc/spatial.hip (max pool / unpool / skip-add,
bilinear and nearest x2, adaptive average pool) and the two per-pixel decoder ops of csrc/pointwise.hip (pixel_gate,
spade_modulate).  Plain helper module (not a conftest, no fixtures), numpy and CPU torch only; nothing here calls an op under test.

Three kinds of function:

* *_ref      -- the operation in fp64 (or exact, for the pool's selection and routing), with the magnitude sums the gates need;
* *_emul     -- the kernel's own fp32 arithmetic in the kernel's grouping, restated in numpy, with the planted defects of
                tests/test_resample_ref.py as keyword switches (all off by default);
* gates      -- gate = (rounding count) * 2^-24 * (magnitude sum of the reference), per element.  The counts are derived beside
                each K_* below from the kernel source; none is fitted.

The shape lists of tests/test_resample_gpu.py live here too, so that the CPU rehearsal (tests/test_resample_ref.py) puts every
emulation through every gate at exactly the shapes the GPU sees."""
import itertools

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24                                  # unit roundoff of fp32 (round to nearest)
TINY = float(np.finfo(np.float32).tiny)         # smallest normal fp32: the absolute term of the bilinear gates
DENORM = 2.0 ** -149                            # spacing of the fp32 subnormals: one rounding of a product that underflows
F32 = np.float32


def f32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32))


def same_bits(a, b):
    """Exact comparison of two fp32 arrays: NaNs are compared as positions, everything else as int32 (so -0.0 != +0.0)."""
    a = f32(a); b = f32(b)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool((na == nb).all() and (a.view(np.int32)[~na] == b.view(np.int32)[~nb]).all())


def worst_ratio(err, gate):
    """max over elements of |err| / gate (0 where both are 0; inf where a zero gate is exceeded; NaN errors count as inf)."""
    err = np.abs(np.asarray(err, dtype=np.float64)); gate = np.asarray(gate, dtype=np.float64) + np.zeros_like(err)
    if err.size == 0:
        return 0.0
    r = np.where(err == 0, 0.0, err / np.where(gate > 0, gate, 1.0))
    r = np.where((err > 0) & (gate <= 0), np.inf, r)
    r = np.where(np.isnan(err) | np.isnan(gate), np.inf, r)
    return float(r.max())


# ============================================================================ bilinear x2, align_corners=True
# Rounding counts (csrc/spatial.hip).  The reference forms l0 = 1 - l1 in fp32 exactly as lerp_coord does, so the weights carry
# no error of their own; l1 = s - i0 is exact (i0 = trunc(s)).
#
# forward, both forms: o = ly0 * (lx0 * v00 + lx1 * v01) + ly1 * (...).  From an input to the result: the product lx * v, the
#   inner sum, the product ly * (.), the outer sum = 4 roundings; the fifth of the issue's count is kept as the cover of the
#   second-order terms ((1 + u)^4 - 1 - 4u) and of magnitudes that A_abs, an exact fp64 sum, understates by a rounding.
K_BIL_FWD = 5
#
# backward, gather form: rowacc = sum over the m_x contributing columns of lx * g, ascending from 0 (one product and m_x - 1
#   sums on the first term's path: m_x roundings), acc = sum over the m_y contributing rows of ly * rowacc (m_y more).  Where
#   i0 == i1 (last output of an axis, or a 1-pixel axis) ONE output adds two terms, one extra sum per axis: (m_x + 1) + (m_y + 1).
# backward, streaming form: the same, plus the rounding of the summed weight lx0 + lx1 where x0 == x1.
def k_bil_bwd(h, w, stream):
    return (contributors(w) + 1) + (contributors(h) + 1) + (1 if stream else 0)


BIL_FWD_BAND = 32                               # output rows per workgroup of the streaming forward
BIL_BWD_BAND = 16                               # input rows per workgroup of the streaming backward


def stream_ok(n, h, w, c):
    """bilinear_stream_ok of csrc/spatial.hip: which of the two forms a shape takes."""
    return c % 16 == 0 and h >= 3 and w >= 3 and n * (2 * h // BIL_FWD_BAND + 1) * (2 * w // 16 + 1) * (c // 16) < (1 << 31)


def lerp_table(n_in, coord='fp32', unrounded=False):
    """(i0, i1, l0, l1) of the 2 * n_in outputs of one axis, formed as lerp_coord forms them: scale = (in - 1) / (2 in - 1) in the
    working type (0 when in == 1), s = scale * o ROUNDED to the working type, i0 = trunc(s) clamped to in - 1,
    i1 = i0 + (i0 < in - 1), l1 = s - i0, l0 = 1 - l1.  coord = 'fp32' is the kernels' arithmetic, 'exact' the same code in fp64.
    unrounded (planted defect): the fp32 scale times o kept unrounded (in fp64, as fma(scale, o, -i0) keeps it), then truncated."""
    ft = {'fp32': np.float32, 'exact': np.float64}[coord]
    n_out = 2 * n_in
    scale = ft(n_in - 1) / ft(n_out - 1) if n_in > 1 else ft(0)
    o = np.arange(n_out)
    if unrounded:
        s = np.float64(scale) * o.astype(np.float64)
        i0 = np.minimum(s.astype(np.int64), n_in - 1)
        l1 = (s - i0).astype(ft)
    else:
        s = scale * o.astype(ft)
        assert s.dtype == ft
        i0 = np.minimum(s.astype(np.int64), n_in - 1)
        l1 = s - i0.astype(ft)
    i1 = i0 + (i0 < n_in - 1)
    l0 = ft(1) - l1
    assert l0.dtype == ft and l1.dtype == ft
    return i0, i1, l0, l1


def _matrix(n_in, coord, **kw):
    i0, i1, l0, l1 = lerp_table(n_in, coord, **kw)
    a = np.zeros((2 * n_in, n_in), dtype=np.float64)
    r = np.arange(2 * n_in)
    np.add.at(a, (r, i0), l0.astype(np.float64))
    np.add.at(a, (r, i1), l1.astype(np.float64))
    return a


def bilinear_matrices(h, w, coord='fp32', **kw):
    """The separable interpolation matrices Ay (2h x h) and Ax (2w x w), float64."""
    return _matrix(h, coord, **kw), _matrix(w, coord, **kw)


def bilinear_ref(x, coord='fp32'):
    """(y, A_abs): y = Ay @ x @ Ax.T per (n, c) in fp64, A_abs = |Ay| @ |x| @ |Ax|.T."""
    x = np.asarray(x, dtype=np.float64)
    ay, ax = bilinear_matrices(x.shape[2], x.shape[3], coord)
    return ay @ x @ ax.T, np.abs(ay) @ np.abs(x) @ np.abs(ax).T


def bilinear_bwd_ref(dy, coord='fp32'):
    """(dx, A_abs): dx = Ay.T @ dy @ Ax per (n, c) in fp64, A_abs = |Ay|.T @ |dy| @ |Ax|."""
    dy = np.asarray(dy, dtype=np.float64)
    ay, ax = bilinear_matrices(dy.shape[2] // 2, dy.shape[3] // 2, coord)
    return ay.T @ dy @ ax, np.abs(ay).T @ np.abs(dy) @ np.abs(ax)


def contributors(n_in):
    """m: the largest number of outputs of one axis that read one input (i0 == i or i1 == i), at most 5 for n_in >= 3."""
    i0, i1, _, _ = lerp_table(n_in)
    return max(int(((i0 == i) | (i1 == i)).sum()) for i in range(n_in))


def bil_gate(k, a_abs):
    return k * U * a_abs + TINY


def bilinear_fwd_emul(x, unrounded=False):
    """Both forward kernels: ly0 * (lx0 * v00 + lx1 * v01) + ly1 * (lx0 * v10 + lx1 * v11) in fp32, every operation rounded."""
    x = f32(x)
    y0, y1, ly0, ly1 = lerp_table(x.shape[2], unrounded=unrounded)
    x0, x1, lx0, lx1 = lerp_table(x.shape[3], unrounded=unrounded)
    r0, r1 = x[:, :, y0], x[:, :, y1]
    h0 = lx0 * r0[..., x0] + lx1 * r0[..., x1]
    h1 = lx0 * r1[..., x0] + lx1 * r1[..., x1]
    out = ly0[:, None] * h0 + ly1[:, None] * h1
    assert out.dtype == np.float32
    return out


def cand_range(i, scale, n_out):
    """cand_range of csrc/spatial.hip in fp32: the candidate outputs scanned for input i."""
    if scale <= 0:
        return 0, n_out - 1
    lo = int(np.floor(F32(i - 1) / scale)) - 1
    hi = int(np.ceil(F32(i + 1) / scale)) + 1
    return max(lo, 0), min(hi, n_out - 1)


def _scale32(n_in):
    return F32(n_in - 1) / F32(2 * n_in - 1) if n_in > 1 else F32(0)


def axis_plan(n_in, summed=False, lo_hi=None, cap=None, drop_fifth=False, drop_carry_of=None):
    """Per input i of one axis: the list of (output o, [weights added in order]) that the backward kernels accumulate, scanning the
    candidate range (lo_hi(i), default cand_range(i)) in ascending order.  summed: the streaming kernel's horizontal form -- one
    weight (x0 == ix ? lx0 : 0) + (x1 == ix ? lx1 : 0) per output, at most `cap` outputs from the first contributing one.
    Planted defects: drop_fifth forgets the fifth contributing output of an input; drop_carry_of = i forgets what input i receives
    as the LOWER neighbour (i1 == i, i0 == i - 1), i.e. what the previous band's rows carry into the first row of a band."""
    i0, i1, l0, l1 = lerp_table(n_in)
    scale = _scale32(n_in)
    plan = []
    for i in range(n_in):
        lo, hi = lo_hi(i) if lo_hi is not None else cand_range(i, scale, 2 * n_in)
        terms, first = [], None
        for o in range(lo, hi + 1):
            if i0[o] != i and i1[o] != i:
                continue
            if first is None:
                first = o
            if cap is not None and o - first >= cap:
                continue
            if drop_fifth and len(terms) == 4:
                continue
            if drop_carry_of == i and i0[o] != i:
                continue
            if summed:
                wts = [(l0[o] if i0[o] == i else F32(0)) + (l1[o] if i1[o] == i else F32(0))]
            else:
                wts = ([l0[o]] if i0[o] == i else []) + ([l1[o]] if i1[o] == i else [])
            terms.append((o, wts))
        plan.append(terms)
    return plan


def _accumulate(g, plan, axis):
    """out[.., i, ..] = sum over plan[i] of weight * g[.., o, ..] along `axis`, fp32, from 0, in plan order."""
    g = np.moveaxis(f32(g), axis, -1)
    out = np.zeros(g.shape[:-1] + (len(plan),), dtype=np.float32)
    for i, terms in enumerate(plan):
        acc = np.zeros(g.shape[:-1], dtype=np.float32)
        for o, wts in terms:
            for wt in wts:
                acc = acc + F32(wt) * g[..., o]
        out[..., i] = acc
    assert out.dtype == np.float32
    return np.moveaxis(out, -1, axis)


def bilinear_bwd_emul(dy, stream, drop_fifth=False, drop_band_row=False):
    """The backward kernels in fp32: acc = sum_oy ly * (sum_ox lx * g), both sums ascending over the scanned candidates.
    stream = False: bilinear_bwd_kernel (cand_range per input row and column, lx0 and lx1 of one output added separately).
    stream = True : bilinear_bwd_stream_kernel (summed last-column weight, <= 5 columns, the row range of the band that owns
    the input row: from cand_range(b0).lo to cand_range(b1 - 1).hi)."""
    dy = f32(dy)
    h, w = dy.shape[2] // 2, dy.shape[3] // 2
    if stream:
        sy = _scale32(h)

        def band_range(iy):
            b0 = iy // BIL_BWD_BAND * BIL_BWD_BAND
            b1 = min(b0 + BIL_BWD_BAND, h)
            return cand_range(b0, sy, 2 * h)[0], cand_range(b1 - 1, sy, 2 * h)[1]
        px = axis_plan(w, summed=True, cap=5, drop_fifth=drop_fifth)
        py = axis_plan(h, lo_hi=band_range, drop_carry_of=BIL_BWD_BAND if drop_band_row else None)
    else:
        px = axis_plan(w, drop_fifth=drop_fifth)
        py = axis_plan(h, drop_carry_of=BIL_BWD_BAND if drop_band_row else None)
    return _accumulate(_accumulate(dy, px, 3), py, 2)


BIL_GATHER_SHAPES = [(3, 8, 3, 520), (1, 4, 2, 1100), (2, 16, 2, 300), (1, 32, 1, 1), (1, 16, 1, 9), (1, 16, 9, 1), (2, 8, 5, 7)]
BIL_STREAM_HW = [(3, 3), (16, 64), (17, 65), (15, 33), (70, 9), (141, 3)]
BIL_STREAM_SHAPES = [(2, c, h, w) for c in (16, 32, 64, 80) for (h, w) in BIL_STREAM_HW] + [(2, 64, 128, 128)]
BIL_CASES = [(s, False) for s in BIL_GATHER_SHAPES] + [(s, True) for s in BIL_STREAM_SHAPES]      # (shape, streaming form expected)


# ============================================================================ nearest x2
NEAREST_SHAPES = [(3, 20, 19, 25), (1, 4, 1, 1), (2, 8, 2, 515)]


def nearest_ref(x):
    return np.repeat(np.repeat(np.asarray(x), 2, axis=2), 2, axis=3)


def nearest_bwd_f32(dy):
    """nearest_bwd_kernel: (a + b) + (c + d) of the four outputs of an input pixel, fp32 (reference and emulation in one: the gate
    is bitwise)."""
    dy = f32(dy)
    a, b, c, d = dy[:, :, 0::2, 0::2], dy[:, :, 0::2, 1::2], dy[:, :, 1::2, 0::2], dy[:, :, 1::2, 1::2]
    out = (a + b) + (c + d)
    assert out.dtype == np.float32
    return out


def nearest_bwd_ref(dy):
    dy = np.asarray(dy, dtype=np.float64)
    return dy[:, :, 0::2, 0::2] + dy[:, :, 0::2, 1::2] + dy[:, :, 1::2, 0::2] + dy[:, :, 1::2, 1::2]


# ============================================================================ max pool 2x2 / unpool
POOL_SHAPES = [(3, 20, 38, 50), (1, 4, 2, 2), (1, 8, 4, 1026), (2, 132, 6, 10)]

_NAN, _INF = float('nan'), float('inf')
# 20 windows (values in scan order k = 2 * dy + dx) whose argmax position cycles 0, 1, 2, 3: the issue's fourteen and six more
# that fill the cycle.  ATen on the CPU: the LAST NaN of a window wins, otherwise the FIRST maximum (all -inf and +-0 ties: 0).
SPECIAL_PATTERNS = [
    ('nan at 0', [_NAN, 1.0, 2.0, 3.0]),
    ('nan at 1', [1.0, _NAN, 2.0, 3.0]),
    ('nan at 2', [1.0, 2.0, _NAN, 3.0]),
    ('nan at 3', [1.0, 2.0, 3.0, _NAN]),
    ('all -inf', [-_INF, -_INF, -_INF, -_INF]),
    ('[nan, nan, 1, 2]', [_NAN, _NAN, 1.0, 2.0]),
    ('[5, nan, nan, 1]', [5.0, _NAN, _NAN, 1.0]),
    ('[1, nan, 5, nan]', [1.0, _NAN, 5.0, _NAN]),
    ('[0, -0, 0, -0]', [0.0, -0.0, 0.0, -0.0]),
    ('[1, 5, 5, 2]', [1.0, 5.0, 5.0, 2.0]),
    ('[1, 2, 5, 5]', [1.0, 2.0, 5.0, 5.0]),
    ('all nan', [_NAN, _NAN, _NAN, _NAN]),
    ('[-0, 0, -0, 0]', [-0.0, 0.0, -0.0, 0.0]),
    ('[-inf, inf, inf, 0]', [-_INF, _INF, _INF, 0.0]),
    ('[-inf, -inf, -0, 0]', [-_INF, -_INF, -0.0, 0.0]),
    ('[inf, inf, 1, nan]', [_INF, _INF, 1.0, _NAN]),
    ('all equal', [2.5, 2.5, 2.5, 2.5]),
    ('[3, 7, 7, 7]', [3.0, 7.0, 7.0, 7.0]),
    ('[1, 2, 9, 3]', [1.0, 2.0, 9.0, 3.0]),
    ('[1, 2, 3, 4]', [1.0, 2.0, 3.0, 4.0]),
]


def rule_argmax(win):
    """The selection rule in plain Python: the last NaN if there is one, else the first maximum."""
    nans = [k for k, v in enumerate(win) if v != v]
    if nans:
        return nans[-1]
    best = 0
    for k in range(1, 4):
        if win[k] > win[best]:
            best = k
    return best


def special_windows():
    """(x, expected): x is (1, 8, 2 R, 2), one window per output row; channel c of window row r holds pattern (r + c) % R, so the
    four lanes of each channel quad hold the four different argmax positions (r + c) % 4 in every row.  expected[r][c] is the
    window byte the rule gives."""
    R = len(SPECIAL_PATTERNS)
    assert R % 4 == 0 and all(rule_argmax(p) == j % 4 for j, (_, p) in enumerate(SPECIAL_PATTERNS))
    x = torch.empty(1, 8, 2 * R, 2, dtype=torch.float32)
    expected = np.zeros((R, 8), dtype=np.uint8)
    for r in range(R):
        for c in range(8):
            win = SPECIAL_PATTERNS[(r + c) % R][1]
            x[0, c, 2 * r:2 * r + 2, :] = torch.tensor(win, dtype=torch.float32).view(2, 2)
            expected[r, c] = rule_argmax(win)
    return x, expected


def special_pattern_at(r, c):
    return SPECIAL_PATTERNS[(r + c) % len(SPECIAL_PATTERNS)][0]


def maxpool_ref(x):
    """(y, k) from stock ATen on the CPU: y fp32 (N, C, OH, OW), k uint8 (N, OH, OW, C) = 2 * (iy - 2 oy) + (ix - 2 ox), the
    kernel's window byte, converted from ATen's flat index."""
    x = torch.as_tensor(x, dtype=torch.float32)
    y, flat = F.max_pool2d(x, 2, 2, return_indices=True)
    n, c, oh, ow = y.shape
    w = x.shape[3]
    iy, ix = flat // w, flat % w
    oy = torch.arange(oh).view(1, 1, oh, 1); ox = torch.arange(ow).view(1, 1, 1, ow)
    k = 2 * (iy - 2 * oy) + (ix - 2 * ox)
    assert int(k.min()) >= 0 and int(k.max()) <= 3
    return y.numpy(), np.ascontiguousarray(k.permute(0, 2, 3, 1).numpy().astype(np.uint8))


def maxpool_emul(x, first_nan=False, last_tie=False, swap_bytes=False):
    """maxpool_fwd_kernel's scan in numpy: best = v[0]; for k = 1..3: if v[k] > best or v[k] != v[k]: take it.
    Planted defects: first_nan (a NaN only displaces a non-NaN), last_tie (>= instead of >), swap_bytes (argmax bytes 0 and 1 of
    every channel quad exchanged in idx)."""
    x = f32(x)
    win = [x[:, :, 0::2, 0::2], x[:, :, 0::2, 1::2], x[:, :, 1::2, 0::2], x[:, :, 1::2, 1::2]]
    best = win[0].copy()
    k = np.zeros(best.shape, dtype=np.uint8)
    with np.errstate(invalid='ignore'):
        for j in range(1, 4):
            v = win[j]
            gt = (v >= best) if last_tie else (v > best)
            take = gt | ((np.isnan(v) & ~np.isnan(best)) if first_nan else np.isnan(v))
            best = np.where(take, v, best); k = np.where(take, np.uint8(j), k)
    k = np.ascontiguousarray(k.transpose(0, 2, 3, 1))
    if swap_bytes:
        k = k.copy(); k[..., 0::4], k[..., 1::4] = k[..., 1::4].copy(), k[..., 0::4].copy()
    return best, k


def scatter_ref(src, k):
    """src (N, C, OH, OW) to the window position k (N, OH, OW, C) of a zero (N, C, 2 OH, 2 OW): pool backward, unpool forward."""
    src = f32(src)
    n, c, oh, ow = src.shape
    kk = k.transpose(0, 3, 1, 2).astype(np.int64)
    out = np.zeros((n, c, 2 * oh, 2 * ow), dtype=np.float32)
    ni, ci, oy, ox = np.meshgrid(np.arange(n), np.arange(c), np.arange(oh), np.arange(ow), indexing='ij')
    out[ni, ci, 2 * oy + (kk >> 1), 2 * ox + (kk & 1)] = src
    return out


def gather_ref(src, k):
    """dst (N, C, OH, OW) = src (N, C, 2 OH, 2 OW) at the window position k: unpool backward."""
    src = f32(src)
    n, c, h, w = src.shape
    kk = k.transpose(0, 3, 1, 2).astype(np.int64)
    ni, ci, oy, ox = np.meshgrid(np.arange(n), np.arange(c), np.arange(h // 2), np.arange(w // 2), indexing='ij')
    return np.ascontiguousarray(src[ni, ci, 2 * oy + (kk >> 1), 2 * ox + (kk & 1)])


def pool_input(shape, seed):
    """Seeded input with what a selection kernel can get wrong everywhere, not in one planted window: values on a grid of 0.5
    (ties in most windows), about 2 % NaN and 1 % -inf."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(shape, generator=g) * 2).round() / 2
    r = torch.rand(shape, generator=g)
    x[r < 0.02] = _NAN
    x[(r >= 0.02) & (r < 0.03)] = -_INF
    return x


# ============================================================================ adaptive average pool -> NCHW-flat
def _avg_cases():
    os_, hws, cs = (1, 2, 6, 7), ((2, 2), (7, 9), (13, 6), (32, 32), (5, 40)), (1, 3, 8, 20)
    cases = [(o, hw, cs[(io + ih) % 4]) for (io, o), (ih, hw) in itertools.product(enumerate(os_), enumerate(hws))]
    cases += [(o, hw, cs[(io + ih + 2) % 4]) for (io, o), (ih, hw) in itertools.product(enumerate(os_), enumerate(hws)) if o >= 6]
    return cases


AVG_N = 3
AVG_CASES = _avg_cases()        # 30 of the 80: every O with every (H, W), every C; H < O, H % O != 0 and W % O != 0 included


def bins(n_in, o, floor_hi=False):
    """[(lo, hi)) of the o bins of one axis: lo = floor(j in / o), hi = ceil((j + 1) in / o).  floor_hi: planted defect."""
    return [((j * n_in) // o, ((j + 1) * n_in) // o if floor_hi else ((j + 1) * n_in + o - 1) // o) for j in range(o)]


def avgpool_ref(x, o):
    """(y, gate): y (N, C o o) fp64 in NCHW-flat order; gate = m * u * (sum |x| / m) per output, m the bin's element count (m - 1
    sums of the sequential accumulation and the divide)."""
    x = np.asarray(x, dtype=np.float64)
    n, c, h, w = x.shape
    y = np.zeros((n, c, o, o)); mag = np.zeros((n, c, o, o))
    for oy, (y0, y1) in enumerate(bins(h, o)):
        for ox, (x0, x1) in enumerate(bins(w, o)):
            m = (y1 - y0) * (x1 - x0)
            y[:, :, oy, ox] = x[:, :, y0:y1, x0:x1].sum(axis=(2, 3)) / m
            mag[:, :, oy, ox] = m * U * (np.abs(x[:, :, y0:y1, x0:x1]).sum(axis=(2, 3)) / m)
    return y.reshape(n, -1), mag.reshape(n, -1)


def avgpool_bwd_ref(dy, shape, o):
    """(dx, gate): dx fp64 (N, C, H, W); gate = (t + 1) * u * sum |dy| / area over the t bins that cover the pixel (the divide and
    the t - 1 sums, one more for the grouping)."""
    n, c, h, w = shape
    dy = np.asarray(dy, dtype=np.float64).reshape(n, c, o, o)
    dx = np.zeros(shape); mag = np.zeros(shape); t = np.zeros((h, w))
    for oy, (y0, y1) in enumerate(bins(h, o)):
        for ox, (x0, x1) in enumerate(bins(w, o)):
            m = (y1 - y0) * (x1 - x0)
            dx[:, :, y0:y1, x0:x1] += (dy[:, :, oy, ox] / m)[:, :, None, None]
            mag[:, :, y0:y1, x0:x1] += (np.abs(dy[:, :, oy, ox]) / m)[:, :, None, None]
            t[y0:y1, x0:x1] += 1
    return dx, (t + 1) * U * mag


def avgpool_emul(x, o, floor_hi=False):
    """avgpool_flat_fwd_kernel: s = 0; s += x over the bin row by row; s / (float) count, fp32."""
    x = f32(x)
    n, c, h, w = x.shape
    y = np.zeros((n, c, o, o), dtype=np.float32)
    with np.errstate(invalid='ignore', divide='ignore'):
        for oy, (y0, y1) in enumerate(bins(h, o, floor_hi)):
            for ox, (x0, x1) in enumerate(bins(w, o, floor_hi)):
                s = np.zeros((n, c), dtype=np.float32)
                for yy in range(y0, y1):
                    for xx in range(x0, x1):
                        s = s + x[:, :, yy, xx]
                y[:, :, oy, ox] = s / F32((y1 - y0) * (x1 - x0))
    return y.reshape(n, -1)


def avgpool_bwd_emul(dy, shape, o, floor_hi=False):
    """avgpool_flat_bwd_kernel: s = 0; for the covering bins in (oy, ox) order: s += dy / (float) area, fp32."""
    n, c, h, w = shape
    dy = f32(dy).reshape(n, c, o, o)
    dx = np.zeros(shape, dtype=np.float32)
    with np.errstate(invalid='ignore', divide='ignore'):
        for oy, (y0, y1) in enumerate(bins(h, o, floor_hi)):
            for ox, (x0, x1) in enumerate(bins(w, o, floor_hi)):
                if y1 > y0 and x1 > x0:
                    dx[:, :, y0:y1, x0:x1] = dx[:, :, y0:y1, x0:x1] + (dy[:, :, oy, ox] / F32((y1 - y0) * (x1 - x0)))[:, :, None, None]
    return dx


# ============================================================================ pixel gate
GATE_CS = (4, 40, 64, 68, 512)
GATE_NHW = ((1, 1, 1), (3, 37, 41), (2, 9, 11))
GATE_CASES = [(n, c, h, w) for c in GATE_CS for (n, h, w) in GATE_NHW]
GATE_TOL = 1e-6            # rtol = atol of tests/test_ops_gpu.py::test_pixel_gate for y and dx: max err <= atol + rtol * max |ref|
GATE_DPSI = 1e-5           # that test's 1e-5 for dpsi, here relative to sum_c |dy x| s (1 - s), per pixel, no absolute term


def gate_inputs(shape, seed):
    n, c, h, w = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, c, h, w, generator=g)
    psi = (torch.randn(n, 1, h, w, generator=g) * 3).clamp(-10, 10)
    dy = torch.randn(n, c, h, w, generator=g)
    return x, psi, dy


def pixel_gate_ref(x, psi, dy):
    """fp64: y = x s, dx = dy s, dpsi = (sum_c dy x) s (1 - s), mag = (sum_c |dy x|) s (1 - s), with s = sigmoid(psi)."""
    x, psi, dy = (np.asarray(t, dtype=np.float64) for t in (x, psi, dy))
    s = 1.0 / (1.0 + np.exp(-psi))
    return dict(y=x * s, dx=dy * s, dpsi=(dy * x).sum(axis=1, keepdims=True) * s * (1 - s),
                mag=np.abs(dy * x).sum(axis=1, keepdims=True) * s * (1 - s))


def close_gate(ref, rtol=GATE_TOL, atol=GATE_TOL):
    """The scalar bound of tests/test_ops_gpu.py::_close: atol + rtol * max |ref|."""
    return atol + rtol * float(np.abs(ref).max())


def pixel_gate_emul(x, psi, dy, first_pass_only=False):
    """pixel_gate_fwd_kernel / pixel_gate_bwd_kernel in fp32: s = 1 / (1 + exp(-psi)); lane sub of 16 accumulates
    (d0 x0 + d1 x1) + (d2 x2 + d3 x3) over the channel quads sub, sub + 16, ...; the lanes fold by xor 8, 4, 2, 1;
    dpsi = acc * s * oms, oms = 1 - s formed as e s for psi >= 0.  first_pass_only (planted defect): the quads cq >= 16 are ignored (dx there is never written)."""
    x, psi, dy = f32(x), f32(psi), f32(dy)
    n, c, h, w = x.shape
    with np.errstate(over='ignore', invalid='ignore'):
        e = np.exp(-psi)
        s = F32(1) / (F32(1) + e)
        oms = np.where(psi >= 0, e * s, F32(1) - s)                 # 1 - s without the cancellation at psi > 0, as the kernel forms it
    assert s.dtype == np.float32 and oms.dtype == np.float32
    cq = c // 4
    prod = (dy * x).reshape(n, cq, 4, h, w)
    quad = (prod[:, :, 0] + prod[:, :, 1]) + (prod[:, :, 2] + prod[:, :, 3])            # (n, cq, h, w)
    lanes = np.zeros((n, 16, h, w), dtype=np.float32)
    for q in range(cq if not first_pass_only else min(cq, 16)):
        lanes[:, q % 16] = lanes[:, q % 16] + quad[:, q]
    for half in (8, 4, 2, 1):
        lanes = lanes[:, :half] + lanes[:, half:2 * half]
    dx = dy * s
    if first_pass_only:
        dx[:, 64:] = 0
    dpsi = lanes * s * oms
    assert dpsi.dtype == np.float32 and dpsi.shape == psi.shape
    return dict(y=x * s, dx=dx, dpsi=dpsi)


# ============================================================================ SPADE modulate
MOD_CASES = [(n, c, h, w) for c in (4, 8, 36, 64) for (n, h, w) in ((2, 6, 6), (3, 37, 41))]


def modulate_inputs(shape, seed):
    n, c, h, w = shape
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, c, h, w, generator=g), torch.randn(n, 2 * c, h, w, generator=g), torch.randn(n, c, h, w, generator=g)


def modulate_ref(x, gb, dy):
    """fp64 y = x (1 + gamma) + beta and its gradients, with the gates:
    y   : 3 u (|x| (1 + |gamma|) + |beta|)   -- 1 + gamma, the product, the sum
    dx  : 2 u |dy| (1 + |gamma|)             -- 1 + gamma, the product
    dgam: u |dy x| (+ one subnormal spacing) -- one product
    dbet: dy itself, bitwise."""
    x, gb, dy = (np.asarray(t, dtype=np.float64) for t in (x, gb, dy))
    c = x.shape[1]
    gam, bet = gb[:, :c], gb[:, c:]
    return dict(y=x * (1 + gam) + bet, y_gate=3 * U * (np.abs(x) * (1 + np.abs(gam)) + np.abs(bet)),
                dx=dy * (1 + gam), dx_gate=2 * U * np.abs(dy) * (1 + np.abs(gam)),
                dgam=dy * x, dgam_gate=U * np.abs(dy * x) + DENORM)


def modulate_emul(x, gb, dy, beta_offset=None):
    """modulate_fwd_kernel / modulate_bwd_kernel in fp32.  beta_offset (planted defect): beta read from that channel offset of
    gamma|beta instead of C."""
    x, gb, dy = f32(x), f32(gb), f32(dy)
    c = x.shape[1]
    off = c if beta_offset is None else beta_offset
    gam, bet = gb[:, :c], gb[:, off:off + c]
    return dict(y=x * (F32(1) + gam) + bet, dx=dy * (F32(1) + gam), dgam=dy * x, dbet=dy.copy())


# ============================================================================ the gates, as error / gate ratios (pass: <= 1)
def bilinear_ratios(x, dy, y, dx, stream):
    n, c, h, w = np.shape(x)
    yr, ya = bilinear_ref(x)
    dr, da = bilinear_bwd_ref(dy)
    return {'fwd': worst_ratio(np.asarray(y, dtype=np.float64) - yr, bil_gate(K_BIL_FWD, ya)),
            'bwd': worst_ratio(np.asarray(dx, dtype=np.float64) - dr, bil_gate(k_bil_bwd(h, w, stream), da))}


def avgpool_ratios(x, o, dy, y, dx):
    yr, yg = avgpool_ref(x, o)
    dr, dg = avgpool_bwd_ref(dy, np.shape(x), o)
    return {'fwd': worst_ratio(np.asarray(y, dtype=np.float64) - yr, yg), 'bwd': worst_ratio(np.asarray(dx, dtype=np.float64) - dr, dg)}


def pixel_gate_ratios(x, psi, dy, got):
    ref = pixel_gate_ref(x, psi, dy)
    return {'y': worst_ratio(np.asarray(got['y'], dtype=np.float64) - ref['y'], close_gate(ref['y'])),
            'dx': worst_ratio(np.asarray(got['dx'], dtype=np.float64) - ref['dx'], close_gate(ref['dx'])),
            'dpsi': worst_ratio(np.asarray(got['dpsi'], dtype=np.float64) - ref['dpsi'], GATE_DPSI * ref['mag'])}


def modulate_ratios(x, gb, dy, got):
    ref = modulate_ref(x, gb, dy)
    out = {k: worst_ratio(np.asarray(got[k], dtype=np.float64) - ref[k], ref[k + '_gate']) for k in ('y', 'dx', 'dgam')}
    out['dbet'] = 0.0 if same_bits(got['dbet'], dy) else float('inf')
    return out
