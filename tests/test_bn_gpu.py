"""csrc/bn.hip against tests/bn_ref.py: the column reductions (statistics, backward sums, channel sum, partial-row fold),
bn_finalize_channel, bn_apply and bn_bwd_apply, fp32 and bf16, entry point by entry point through the C-ABI and assembled through
ops.batch_norm_act / bf16.batch_norm_act.  tests/test_bn_ref.py rehearses every gate used here on the CPU: an emulation of each
kernel passes it at these very cases, and each planted defect fails it.

Every gate is exact (bits) or a rounding count times a unit roundoff times a magnitude sum of the fp64 reference; the counts are
derived in bn_ref.py beside each gate.  No case is filtered by value: the all-zero, constant and mean^2/var = 1e10 channels are compared.

What the file states that nothing stated before:
* fp64 accumulation keeps E[x^2] - mean^2 alive at mean^2 / var = 1e10 (every statistics case has such a channel);
* two runs give the same bits (no atomics, fixed order), the fused finalize route and the two-launch route give the same bits;
* workspaces are used at exactly the queried size (NaN-filled, guard band behind), for every geometry edge of red_geom;
* scale / shift / running_mean / running_var are the specified function (explicit fmas) of the kernel's mean / invstd / sums, bit for bit;
* the backward's recomputed activation mask equals the forward's y > 0 for pre-activations within rounding of zero, bit for bit;
* the > 48 KiB dynamic-LDS opt-in of bn_bwd_apply at P <= 32, up to the documented C = 4096;
* the sync-BN count riding in sums[2C], without a process group; var_mode 1 clamping instead of adding eps.

No defect was found in bn.hip: every case passes, the C = 4096 launch with 160 KiB of dynamic LDS included.  Two gates are
re-derived in bn_ref.py, wider than first stated: bf16 keeps 8 significand bits, so a correct round-to-nearest store errs by up to
2^-8 |value|, not 2^-9 (tests/test_bn_ref.py::test_bf16_unit_roundoff; the truncating store still fails it, 1.94); and LeakyReLU's
negative side is the fp32 product v * slope, one rounding more than ReLU (counted on that side only).

Worst measured error / gate per family on an MI355X (pass: <= 1; the CPU rehearsal's figure in brackets):

    statistics fp32             0.00 s1, 0.19 s2, 1.00 mean, 0.995 invstd, 1.00 channel sum      [0.00, 0.19, 1.00, 0.995, 0.90]
    statistics bf16             0.0003 s1, 0.04 s2, 0.39 mean, 0.70 invstd                       [0.0003, 0.04, 0.39, 0.70]
    scale / shift / running_mean / running_var, recomputed mask, two runs, fused vs two-launch: exact
    partial rows                0.14 s1, 0.11 s2                                                 [0.14, 0.11]
    finalize (given sums)       0.96 mean, 0.95 invstd
    sync-BN shards              0.93 mean, 0.70 invstd, 0.01 backward sums, 0.995 dx
    apply                       0.63 fp32, 0.49 fp32 swish, 0.996 bf16 and bf16 swish             [0.63, 0.45, 0.996, 0.996]
    backward fp32               0.05 sums, 0.99 dweight, 1.00 dbias, 1.00 dx, dres exact         [0.05, 0.99, 1.00, 1.00]
              swish             0.37 sums, 0.57 dres, 0.95 dx                                    [0.51, 0.64, 0.93]
    backward bf16               0.47 sums, 0.50 dbias, 0.996 dx, dres exact                      [0.47, 0.44, 0.996]
              swish             0.34 sums, 0.99 dres, 0.996 dx                                   [0.43, 0.99, 0.996]
    assembled fp32              0.60 y, 0.93 dx, 0.97 dbias, 0.16 dweight, 0.82 running_mean, 0.38 running_var
    assembled bf16              0.995 y, 0.995 dx, 0.04 dbias, 0.02 dweight

  (mean, dx, dbias, the channel sum and the bf16 stores are single roundings of an accurately known value: a half-ulp bound is met at 1.00.)

In one run of the whole GPU suite the file's 175 cases take 30 s (the largest, the 34-MB bf16 clamp shapes, 4.6 s each, most of it
the fp64 reference on the host); in the same run tests/test_resample_gpu.py's 94 cases take under 2 s (0.4 s in tests above 20 ms)
and tests/test_ops_gpu.py 8 s.
"""
import ctypes as C_

import numpy as np
import pytest
import torch

import bn_ref as br
from bn_ref import ACT_LRELU, ACT_NONE, ACT_RELU, ACT_SWISH, F32, F64, f32

pytestmark = pytest.mark.gpu

SLOPE = 0.2
GUARD = 512                                              # bytes of guard band behind a workspace
POISON = 0xA5
BF = torch.bfloat16


def _report(family, ratios):
    print('RATIO %-28s %s' % (family, '  '.join('%s=%.3g' % kv for kv in sorted(ratios.items()))))


def _ok(ratios):
    return all(v <= 1.0 for v in ratios.values())


def _np(t):
    t = t.detach()
    return np.ascontiguousarray((t.float() if t.dtype == BF else t).cpu().numpy())


def _to(a, dev, bf16=False):
    t = torch.from_numpy(np.array(a, order="C")).to(dev)
    return t.to(BF) if bf16 else t


def _sfx(bf16):
    return '_bf16' if bf16 else '_f32'


def _id(c):
    return '%dx%d' % tuple(c[:2])


class _Ws(object):
    """A workspace of exactly `nbytes`, NaN-filled (a partial row that is read but never written shows), with a poisoned guard band
    behind it that must survive."""

    def __init__(self, nbytes, dev):
        self.n = int(nbytes)
        assert self.n % 8 == 0
        self.buf = torch.empty(self.n + GUARD, dtype=torch.uint8, device=dev)
        assert self.buf.data_ptr() % 16 == 0
        self.fill()

    def fill(self):
        self.buf[:self.n].view(torch.float64).fill_(float('nan'))
        self.buf[self.n:] = POISON

    def ptr(self):
        return C_.c_void_p(self.buf.data_ptr())

    def intact(self):
        return bool((self.buf[self.n:] == POISON).all().item())


class _Abi(object):
    """The C-ABI entry points of bn.hip over [P, C] row tensors, one method each; pointers, strides and the stream filled in."""

    def __init__(self, pkg, dev):
        self.lib, self.ops, self.dev = pkg._lib, pkg.ops, dev

    def call(self, name, *a):
        return self.lib.call(name, *(a + (self.lib.stream_ptr(),)))

    def ws(self, P, C):
        return _Ws(self.lib.call('ssg_bn_workspace_bytes', P, C), self.dev)

    def stats(self, x, P, C, ld, bf16, ws, with_count=1):
        sums = torch.full((2 * C + 1,), float('nan'), dtype=torch.float64, device=self.dev)
        self.call('ssg_bn_stats' + _sfx(bf16), self.lib.ptr(x), P, C, ld, self.lib.ptr(sums), with_count, ws.ptr())
        return sums

    def fin_struct(self, C, weight, bias, eps, momentum, var_mode, rm, rv):
        stats = torch.full((4, C), float('nan'), dtype=torch.float32, device=self.dev)
        return self.ops.bn_fin(weight, bias, eps, momentum, var_mode, rm, rv, stats), stats

    def finalize(self, sums, count, C, weight, bias, eps, momentum, var_mode, rm, rv):
        p = self.lib.ptr
        stats = torch.full((4, C), float('nan'), dtype=torch.float32, device=self.dev)
        self.call('ssg_bn_finalize_f32', p(sums), float(count), C, p(weight), p(bias), eps, momentum, var_mode, p(rm), p(rv),
                  p(stats[0]), p(stats[1]), p(stats[2]), p(stats[3]))
        return stats

    def stats_finalize(self, x, P, C, ld, bf16, ws, weight, bias, eps, momentum, var_mode, rm, rv):
        fin, stats = self.fin_struct(C, weight, bias, eps, momentum, var_mode, rm, rv)
        self.call('ssg_bn_stats_finalize' + _sfx(bf16), self.lib.ptr(x), P, C, ld, C_.byref(fin), ws.ptr())
        return stats

    def apply(self, x, P, C, ld, scale, shift, res, ldr, act, slope, bf16, out=None):
        """`out`: (view, ld) of a wider buffer to write into; default a fresh dense [P, C]."""
        p = self.lib.ptr
        y, ldy = out if out is not None else (torch.full((P, C), float('nan'), dtype=BF if bf16 else torch.float32, device=self.dev), C)
        self.call('ssg_bn_apply' + _sfx(bf16), p(x), P, C, ld, p(scale), p(shift), p(res), ldr, act, slope, p(y), ldy)
        return y

    def bwd_reduce(self, x, y, dy, P, C, ld, mean, invstd, scale, shift, act, slope, bf16, ws, with_count=0, lds=None):
        p = self.lib.ptr
        ldx, ldy, lddy = lds or (ld, ld, ld)
        sums = torch.full((2 * C + 1,), float('nan'), dtype=torch.float64, device=self.dev)
        self.call('ssg_bn_bwd_reduce' + _sfx(bf16), p(x), p(y), p(dy), P, C, ldx, ldy if y is not None else 0, lddy, p(mean), p(invstd),
                  p(scale), p(shift), act, slope, p(sums), with_count, ws.ptr())
        return sums

    def bwd_apply(self, x, y, dy, P, C, ld, mean, invstd, weight, scale, shift, sums, count, act, slope, bf16, want_dx=True, want_dres=True,
                  lds=None, outs=None):
        """`outs`: ((dx view, lddx), (dres view, lddres)) of wider buffers; default fresh dense [P, C] tensors."""
        p = self.lib.ptr
        ldx, ldy, lddy = lds or (ld, ld, ld)
        dt = BF if bf16 else torch.float32
        fresh = lambda want: (torch.full((P, C), float('nan'), dtype=dt, device=self.dev), C) if want else (None, 0)
        (dx, lddx), (dres, lddres) = outs if outs is not None else (fresh(want_dx), fresh(want_dres))
        dwb = torch.full((2, C), float('nan'), dtype=torch.float32, device=self.dev)
        self.call('ssg_bn_bwd_apply' + _sfx(bf16), p(x), p(y), p(dy), P, C, ldx, ldy if y is not None else 0, lddy, p(mean), p(invstd), p(weight),
                  p(scale), p(shift), p(sums), float(count), act, slope, p(dx), lddx, p(dres), lddres,
                  p(dwb[0]), p(dwb[1]))
        return dx, dres, dwb[0], dwb[1]


@pytest.fixture()
def abi(pkg, dev):
    return _Abi(pkg, dev)


# ----------------------------------------------------------------------------- 1. statistics
@pytest.mark.parametrize('bf16,case', [(False, c) for c in br.STAT_CASES_F32] + [(True, c) for c in br.STAT_CASES_BF16],
                         ids=lambda v: _id(v) if isinstance(v, tuple) else ('bf16' if v else 'f32'))
def test_statistics(abi, dev, bf16, case):
    P, C = case[:2]
    eps, var_mode, mom = (1e-5 if P % 2 else 1e-3), (P // 2) % 2, 0.1
    x = br.stats_data(P, C, 3, bf16)
    ref = br.stats_ref(x)
    w, b = br.affine_data(C, 4)
    xd, wd, bd = _to(x, dev, bf16), _to(w, dev), _to(b, dev)
    ws = abi.ws(P, C)
    runs = []
    for _ in range(2):                                   # twice: no atomics, fixed order -> the same bits
        ws.fill()
        sums = abi.stats(xd, P, C, C, bf16, ws)
        ws.fill()
        rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
        fused = abi.stats_finalize(xd, P, C, C, bf16, ws, wd, bd, eps, mom, var_mode, rm, rv)
        runs.append((_np(sums), _np(fused), _np(rm), _np(rv)))
    assert ws.intact(), 'guard band behind the workspace'
    for a, bb in zip(runs[0], runs[1]):
        assert np.array_equal(a.view(np.int64 if a.dtype == F64 else np.int32), bb.view(np.int64 if bb.dtype == F64 else np.int32)), 'two runs differ'
    sums, fused, rm_f, rv_f = runs[0]
    assert sums[2 * C] == float(P)                       # with_count: the pixel count rides behind the sums
    s1, s2 = sums[:C], sums[C:2 * C]
    r = br.stats_ratios(x, s1, s2, bf16, ref)
    # the two-launch route on those sums: the same bits as the fused route
    rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    two = _np(abi.finalize(_to(sums, dev), P, C, wd, bd, eps, mom, var_mode, rm, rv))
    assert br.same_bits(two, fused) and br.same_bits(_np(rm), rm_f) and br.same_bits(_np(rv), rv_f), 'fused and two-launch finalize differ'
    mean, invstd = fused[0], fused[1]
    r.update(br.moment_ratios(ref, mean, invstd, br.sum_rel(P, C, bf16), eps, var_mode))
    r.update(br.exact_ratios(dict(scale=fused[2], shift=fused[3], running_mean=rm_f), mean, invstd, w, b, mom, np.zeros(C, F32)))
    r['running_var'] = 0.0 if br.same_bits(rv_f, br.running_var_exact(s1, s2, P, mom, np.ones(C, F32))[0]) else float('inf')
    if not bf16:
        ws.fill()
        out = torch.full((C,), float('nan'), device=dev)
        abi.call('ssg_channel_sum_f32', abi.lib.ptr(xd), P, C, C, abi.lib.ptr(out), ws.ptr())
        g = br.sum_gate(P, C, ref['a1'])
        r['fsum'] = br.worst_ratio(_np(out).astype(F64) - ref['s1'], g + br.U32 * (np.abs(ref['s1']) + g) + br.DENORM)
        assert br.same_bits(_np(out), s1.astype(F32)) and ws.intact()       # the same reduction, rounded once
    _report('statistics %s %s' % ('bf16' if bf16 else 'f32', _id(case)), r)
    assert _ok(r), r


@pytest.mark.parametrize('P,C', br.CHANNEL_SUM_EXTRA)
def test_channel_sum_odd_channels(abi, dev, P, C):
    ld = (C + 3) // 4 * 4 + 4
    x = br.stats_data(P, C, 5)
    xd = torch.full((P, ld), float('nan'), device=dev)                      # lanes beyond C in the last quad hold NaN: they must not be summed
    xd[:, :C] = _to(x, dev)
    ws = abi.ws(P, C)
    out = torch.full((C + 4,), -7.0, device=dev)
    abi.call('ssg_channel_sum_f32', abi.lib.ptr(xd), P, C, ld, abi.lib.ptr(out), ws.ptr())
    ref = br.stats_ref(x)
    g = br.sum_gate(P, C, ref['a1'])
    got = _np(out)
    r = {'fsum': br.worst_ratio(got[:C].astype(F64) - ref['s1'], g + br.U32 * (np.abs(ref['s1']) + g) + br.DENORM)}
    _report('channel sum %dx%d' % (P, C), r)
    assert _ok(r) and (got[C:] == -7.0).all() and ws.intact()


# ----------------------------------------------------------------------------- 2. partial rows
@pytest.mark.parametrize('rows,C', br.PARTIAL_CASES)
def test_partial_rows(abi, dev, rows, C):
    lib = abi.lib
    part = br.partial_rows(rows, C, rows)
    pd = _to(part, dev)
    count = 8.0 * rows
    ws = _Ws(lib.call('ssg_bn_stats_from_partials_workspace_bytes', rows, C), dev)
    w, b = br.affine_data(C, 6)
    wd, bd = _to(w, dev), _to(b, dev)
    runs = []
    for _ in range(2):
        ws.fill()
        sums = torch.full((2 * C + 1,), float('nan'), dtype=torch.float64, device=dev)
        abi.call('ssg_bn_stats_from_partials_f32', lib.ptr(pd), rows, C, lib.ptr(sums), count, ws.ptr())
        ws.fill()
        rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
        fin, stats = abi.fin_struct(C, wd, bd, 1e-5, 0.1, 0, rm, rv)
        abi.call('ssg_bn_stats_from_partials_finalize_f32', lib.ptr(pd), rows, C, count, C_.byref(fin), ws.ptr())
        runs.append((_np(sums), _np(stats), _np(rm), _np(rv)))
    assert ws.intact()
    for a, bb in zip(runs[0], runs[1]):
        assert a.tobytes() == bb.tobytes(), 'two runs differ'
    sums, fused, rm_f, rv_f = runs[0]
    assert sums[2 * C] == count
    r = br.partials_ratios(part, sums[:C], sums[C:2 * C])
    rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    two = _np(abi.finalize(_to(sums, dev), count, C, wd, bd, 1e-5, 0.1, 0, rm, rv))
    assert br.same_bits(two, fused) and br.same_bits(_np(rm), rm_f) and br.same_bits(_np(rv), rv_f), 'fused and two-launch routes differ'
    _report('partial rows %dx%d' % (rows, C), r)
    assert _ok(r), r


# ----------------------------------------------------------------------------- 3. finalize
@pytest.mark.parametrize('var_mode', [0, 1])
@pytest.mark.parametrize('eps', [1e-5, 1e-3])
@pytest.mark.parametrize('momentum', [0.1, 0.01])
def test_finalize(abi, dev, var_mode, eps, momentum):
    P, C = 319, 260
    x = br.stats_data(P, C, 8)
    ref = br.stats_ref(x)
    w, b = br.affine_data(C, 9)
    rm0 = f32(np.random.RandomState(10).standard_normal(C)); rv0 = f32(np.random.RandomState(11).rand(C) + 0.5)
    worst = {}
    for affine, running, count_arg in ((True, True, P), (False, True, P), (True, False, P), (True, True, 0)):
        sums = np.concatenate([ref['s1'], ref['s2'], [float(P)]])
        wd, bd = (_to(w, dev), _to(b, dev)) if affine else (None, None)
        rm, rv = (_to(rm0, dev), _to(rv0, dev)) if running else (None, None)
        st = _np(abi.finalize(_to(sums, dev), count_arg, C, wd, bd, eps, momentum, var_mode, rm, rv))       # count_arg 0: sums[2C] is read
        r = br.moment_ratios(ref, st[0], st[1], 2 * br.U64, eps, var_mode)
        got = dict(scale=st[2], shift=st[3])
        if running:
            got['running_mean'] = _np(rm)
            r['running_var'] = 0.0 if br.same_bits(_np(rv), br.running_var_exact(ref['s1'], ref['s2'], P, momentum, rv0)[0]) else float('inf')
        r.update(br.exact_ratios(got, st[0], st[1], w if affine else None, b if affine else None, momentum, rm0 if running else None))
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)
    # count == 1: a single pixel, the running variance takes the biased value (no division by zero)
    x1 = br.stats_data(1, C, 12)
    r1 = br.stats_ref(x1)
    rm, rv = _to(rm0, dev), _to(rv0, dev)
    st = _np(abi.finalize(_to(np.concatenate([r1['s1'], r1['s2'], [1.0]]), dev), 1, C, _to(w, dev), _to(b, dev), eps, momentum, var_mode, rm, rv))
    assert np.isfinite(_np(rv)).all() and br.same_bits(_np(rv), br.running_var_exact(r1['s1'], r1['s2'], 1, momentum, rv0)[0])
    assert br.same_bits(st[0], x1[0]) and _ok(br.moment_ratios(r1, st[0], st[1], 2 * br.U64, eps, var_mode))
    _report('finalize vm%d eps%g mom%g' % (var_mode, eps, momentum), worst)
    assert _ok(worst), worst


# ----------------------------------------------------------------------------- 4. sync-BN arithmetic without a process group
@pytest.mark.parametrize('bf16', [False, True], ids=['f32', 'bf16'])
def test_sync_bn_arithmetic_two_unequal_shards(abi, dev, bf16):
    H, W, C = 13, 11, 40
    eps, var_mode = 1e-5, 1
    n = 8 * H * W
    x = br.stats_data(n, C, 14, bf16); dy = br.grad_data(n, C, 15, bf16)
    cut = 3 * H * W
    w, b = br.affine_data(C, 16)
    wd, bd = _to(w, dev), _to(b, dev)
    shards = [(x[:cut], dy[:cut]), (x[cut:], dy[cut:])]
    total = torch.zeros(2 * C + 1, dtype=torch.float64, device=dev)
    for xs, _ in shards:
        P = xs.shape[0]
        total += abi.stats(_to(xs, dev, bf16), P, C, C, bf16, abi.ws(P, C), with_count=1)             # what the all-reduce would do
    assert _np(total)[2 * C] == float(n)
    st = abi.finalize(total, 0, C, wd, bd, eps, 0.1, var_mode, None, None)                           # count 0: read sums[2C]
    stn = _np(st)
    ref = br.stats_ref(x)
    k_rel = max(br.sum_rel(s[0].shape[0], C, bf16) for s in shards) + br.U64                          # + the one addition of the two shards
    r = br.moment_ratios(ref, stn[0], stn[1], k_rel, eps, var_mode)
    r.update(br.exact_ratios(dict(scale=stn[2], shift=stn[3]), stn[0], stn[1], w, b, 0.1, None))
    # backward: per-shard reduce with the count, host add, apply with count = 0
    y = [abi.apply(_to(xs, dev, bf16), xs.shape[0], C, C, st[2], st[3], None, 0, ACT_RELU, 0.0, bf16) for xs, _ in shards]
    tot_b = torch.zeros(2 * C + 1, dtype=torch.float64, device=dev)
    for (xs, ds), ys in zip(shards, y):
        P = xs.shape[0]
        tot_b += abi.bwd_reduce(_to(xs, dev, bf16), ys, _to(ds, dev, bf16), P, C, C, st[0], st[1], st[2], st[3], ACT_RELU, 0.0, bf16, abi.ws(P, C), 1)
    tb = _np(tot_b)
    assert tb[2 * C] == float(n)
    y_all = np.concatenate([_np(t) for t in y])
    dxs = [abi.bwd_apply(_to(xs, dev, bf16), ys, _to(ds, dev, bf16), xs.shape[0], C, C, st[0], st[1], wd, st[2], st[3], tot_b, 0, ACT_RELU, 0.0,
                         bf16, want_dres=False)[0] for (xs, ds), ys in zip(shards, y)]
    dx = np.concatenate([_np(t) for t in dxs])
    # gate of the summed sums: each shard's own chain, the shards' magnitudes add up to the whole's
    rb = br.bwd_ratios(x, dy, y_all > 0, stn[0], stn[1], w, stn[2], stn[3], ACT_RELU, 0.0, n, tb[:C], tb[C:2 * C], dx=dx, bf16=bf16)
    r.update({'bwd_' + k: v for k, v in rb.items()})
    _report('sync-BN shards %s' % ('bf16' if bf16 else 'f32'), r)
    assert _ok(r), r


# ----------------------------------------------------------------------------- 5. apply
APPLY_F32 = [(1, 4), (3, 4), (767, 40), (319, 260), (32773, 256)]
APPLY_BF16 = [(1, 8), (1023, 24), (159, 520), (32773, 512)]
ACT_RES = [(ACT_NONE, False), (ACT_NONE, True), (ACT_RELU, False), (ACT_RELU, True), (ACT_LRELU, False), (ACT_LRELU, True), (ACT_SWISH, False)]
BIG_ACT_RES = [(ACT_LRELU, True), (ACT_SWISH, False)]    # the 34-MB shapes are there for the grid, not for the activation list


@pytest.mark.parametrize('bf16,P,C', [(False,) + s for s in APPLY_F32] + [(True,) + s for s in APPLY_BF16])
def test_apply(abi, dev, bf16, P, C):
    x = br.stats_data(P, C, 7, bf16)
    _, _, _, _, scale, shift = br.bwd_consts(x, C, 8)
    res = br.grad_data(P, C, 9, bf16)
    xd, rd, scd, shd = _to(x, dev, bf16), _to(res, dev, bf16), _to(scale, dev), _to(shift, dev)
    worst = {}
    for act, with_res in (ACT_RES if P * C < br.BIG else BIG_ACT_RES):
        y = _np(abi.apply(xd, P, C, C, scd, shd, rd if with_res else None, C if with_res else 0, act, SLOPE, bf16))
        if act == ACT_SWISH:
            assert np.abs(br.apply_ref(x, scale, shift, None, act, SLOPE)[1]).max() <= 10
        r = br.apply_ratios(x, scale, shift, res if with_res else None, act, SLOPE, y, bf16)
        key = 'swish' if act == ACT_SWISH else 'y'
        worst[key] = max(worst.get(key, 0.0), r['y'])
    with pytest.raises(abi.lib.HipLibraryError):
        abi.apply(xd, P, C, C, scd, shd, rd, C, ACT_SWISH, 0.0, bf16)                                 # swish with a residual is refused
    _report('apply %s %dx%d' % ('bf16' if bf16 else 'f32', P, C), worst)
    assert _ok(worst), worst


@pytest.mark.parametrize('bf16', [False, True], ids=['f32', 'bf16'])
def test_swish_limits(abi, dev, bf16):
    """|z| in {20, 90, 104}: only the limits -- finite, y -> z and swish' -> 1 on one side, y -> -0 and swish' -> 0 on the other."""
    C = 8
    zs = np.array([20.0, -20.0, 90.0, -90.0, 104.0, -104.0, 20.0, -104.0], dtype=F32)
    x = np.tile(zs, (3, 1))
    one, zero = torch.ones(C, device=dev), torch.zeros(C, device=dev)
    xd = _to(x, dev, bf16)
    y = _np(abi.apply(xd, 3, C, C, one, zero, None, 0, ACT_SWISH, 0.0, bf16))
    sums = torch.zeros(2 * C + 1, dtype=torch.float64, device=dev)
    dy = _to(np.ones((3, C), F32), dev, bf16)
    _, d, _, _ = abi.bwd_apply(xd, None, dy, 3, C, C, zero, one, None, one, zero, sums, 3, ACT_SWISH, 0.0, bf16, want_dx=False)
    d = _np(d)
    for j, z in enumerate(zs):
        assert br.swish_limit_ok(z, y[0, j], d[0, j], br.UBF if bf16 else 0.0), (z, y[0, j], d[0, j])


def test_affine_act_eval_padded_lanes(pkg, dev):
    """_AffineAct (eval mode) at C in {1, 3}, the psi norm's padded lanes: the values, and the pad lanes stay 0."""
    ops = pkg.ops
    for c in (1, 3):
        bn = torch.nn.BatchNorm2d(c).to(dev)
        g = torch.Generator().manual_seed(20 + c)
        with torch.no_grad():
            bn.weight.copy_(torch.rand(c, generator=g) + 0.5); bn.bias.copy_(torch.randn(c, generator=g))
            bn.running_mean.copy_(torch.randn(c, generator=g)); bn.running_var.copy_(torch.rand(c, generator=g) + 0.5)
        bn.eval()
        x = torch.randn(2, c, 5, 7, generator=g)
        for act in (ACT_NONE, ACT_RELU, ACT_LRELU):
            y = ops.batch_norm_act(x.to(dev), bn, act=act, slope=SLOPE)
            with torch.no_grad():                        # the constants as batch_norm_act forms them, with the same torch ops on the device
                sc = torch.rsqrt(bn.running_var + bn.eps) * bn.weight
                scale, shift = _np(sc), _np(-bn.running_mean * sc + bn.bias)
            rows = np.ascontiguousarray(x.permute(0, 2, 3, 1).reshape(-1, c).numpy())
            got = np.ascontiguousarray(_np(y).transpose(0, 2, 3, 1).reshape(-1, c))
            assert _ok(br.apply_ratios(rows, scale, shift, None, act, SLOPE, got))
            raw = torch.empty(0, device=dev).set_(y.untyped_storage(), 0, (2 * 5 * 7, 4), (4, 1))
            assert (raw[:, c:] == 0).all().item(), 'pad lanes of the eval-mode output'
        assert bn.num_batches_tracked.item() == 0


# ----------------------------------------------------------------------------- 6. mask consistency, exact
@pytest.mark.parametrize('bf16', [False, True], ids=['f32', 'bf16'])
@pytest.mark.parametrize('act', [ACT_RELU, ACT_LRELU])
def test_recomputed_mask_is_the_forward_mask(abi, dev, bf16, act):
    """All 36 864 fp32 pre-activations lie within rounding of zero.  A bf16 ulp of x is 2^16 fp32 ulps of the product, so of the bf16
    probe only the two step-0 rows (4096 elements) can flip; the other rows check the plain mask."""
    C, P = 2048, 18
    x, scale, shift = br.mask_probe(C, P, 21, bf16)
    slope = SLOPE if act == ACT_LRELU else 0.0
    xd, scd, shd = _to(x, dev, bf16), _to(scale, dev), _to(shift, dev)
    y = abi.apply(xd, P, C, C, scd, shd, None, 0, act, slope, bf16)
    pos = _np(y) > 0
    assert pos.any() and (~pos).any()
    dy = _to(np.ones((P, C), F32), dev, bf16)
    zero, one = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    off = F32(0) if act == ACT_RELU else (br.bf16_rne(np.array([SLOPE], F32))[0] if bf16 else F32(SLOPE))
    want = np.where(pos, F32(1), off)
    ws = abi.ws(P, C)
    got = {}
    for route, yy in (('recomputed', None), ('from y', y)):
        sums = abi.bwd_reduce(xd, yy, dy, P, C, C, zero, one, scd, shd, act, slope, bf16, ws)
        _, dres, _, _ = abi.bwd_apply(xd, yy, dy, P, C, C, zero, one, None, scd, shd, sums, P, act, slope, bf16, want_dx=False)
        got[route] = (_np(sums)[:C], _np(dres))
        n_bad = int((got[route][1] != want).sum())
        assert n_bad == 0, '%s: %d of %d masks differ from y > 0' % (route, n_bad, P * C)
        cnt = pos.sum(axis=0).astype(F64)
        if act == ACT_RELU:                              # sums[0:C] = sum of the masked dy = the per-channel count of the mask, exactly
            assert np.array_equal(got[route][0], cnt), route
        else:                                            # count + (P - count) * fl32(slope): at most 18 such terms are exact in fp64 (fp32
            tot = cnt + (P - cnt) * float(F32(SLOPE))    # tensors); a bf16 tensor's thread adds them in fp32, gated as any bf16 column sum
            if bf16:
                assert br.worst_ratio(got[route][0] - tot, br.sum_gate(P, C, tot, True)) <= 1.0, route
            else:
                assert np.array_equal(got[route][0], tot), route
    assert got['recomputed'][0].tobytes() == got['from y'][0].tobytes() and br.same_bits(got['recomputed'][1], got['from y'][1])


# ----------------------------------------------------------------------------- 7. backward
def _backward_case(abi, dev, P, C, bf16, tag):
    x = br.stats_data(P, C, 11, bf16)
    dy = br.grad_data(P, C, 12, bf16)
    w, b, mean, invstd, scale, shift = br.bwd_consts(x, C, 13)
    xd, dyd = _to(x, dev, bf16), _to(dy, dev, bf16)
    wd, md, isd, scd, shd = (_to(a, dev) for a in (w, mean, invstd, scale, shift))
    ws = abi.ws(P, C)
    worst = {}
    # (activation, mask from y?, weight given?, dx wanted?, dres wanted?)
    plans = [(ACT_NONE, False, True, True, False), (ACT_RELU, True, False, True, True), (ACT_LRELU, False, True, False, True)]
    plans += [(ACT_SWISH, False, True, True, True)]
    if P * C >= br.BIG:                                  # the 34-MB shapes are there for the geometry: one mask plan with every output, and swish
        plans = [(ACT_RELU, True, True, True, True), plans[-1]]
    for act, with_y, with_w, want_dx, want_dres in plans:
        slope = SLOPE if act == ACT_LRELU else 0.0
        y = abi.apply(xd, P, C, C, scd, shd, None, 0, act, slope, bf16)
        ws.fill()
        sums = abi.bwd_reduce(xd, y if with_y else None, dyd, P, C, C, md, isd, scd, shd, act, slope, bf16, ws)
        dx, dres, dwt, dbs = abi.bwd_apply(xd, y if with_y else None, dyd, P, C, C, md, isd, wd if with_w else None, scd, shd, sums, P, act,
                                           slope, bf16, want_dx, want_dres)
        sn = _np(sums)
        r = br.bwd_ratios(x, dy, _np(y) > 0, mean, invstd, w if with_w else None, scale, shift, act, slope, P, sn[:C], sn[C:2 * C],
                          dx=_np(dx) if want_dx else None, dres=_np(dres) if want_dres else None, dweight=_np(dwt), dbias=_np(dbs), bf16=bf16)
        for k, v in r.items():
            k = ('swish_' + k) if act == ACT_SWISH else k
            worst[k] = max(worst.get(k, 0.0), v)
    assert ws.intact()
    _report('backward %s %s' % ('bf16' if bf16 else 'f32', tag), worst)
    assert _ok(worst), worst


@pytest.mark.parametrize('bf16,case', [(False, c) for c in br.BWD_CASES_F32] + [(True, c) for c in br.BWD_CASES_BF16],
                         ids=lambda v: _id(v) if isinstance(v, tuple) else ('bf16' if v else 'f32'))
def test_backward(abi, dev, bf16, case):
    _backward_case(abi, dev, case[0], case[1], bf16, _id(case))


@pytest.mark.parametrize('bf16,case', [(False, c) for c in br.LDS_CASES] + [(True, c) for c in br.LDS_CASES_BF16],
                         ids=lambda v: _id(v) if isinstance(v, tuple) else ('bf16' if v else 'f32'))
def test_backward_dynamic_lds(abi, dev, bf16, case):
    """bn_bwd_apply keeps 5 C doubles in LDS: 48 KiB is passed at C = 1232 (hipFuncSetAttribute opt-in), C = 4096 is 160 KiB exactly."""
    _backward_case(abi, dev, case[0], case[1], bf16, _id(case) + (' opt-in' if case[2] else ''))


def test_backward_refuses_more_than_4096_channels(abi, dev):
    P, C = 2, br.LDS_REFUSED_C
    z = torch.zeros((P, C), device=dev); v = torch.ones(C, device=dev)
    sums = torch.zeros(2 * C + 1, dtype=torch.float64, device=dev)
    with pytest.raises(abi.lib.HipLibraryError):
        abi.bwd_apply(z, None, z, P, C, C, v, v, v, v, v, sums, P, ACT_NONE, 0.0, False)


@pytest.mark.parametrize('bf16', [False, True], ids=['f32', 'bf16'])
def test_channel_slice_of_a_wider_tensor(abi, dev, bf16):
    """ld > C at every entry point, fp32 and bf16: x, y, dy, dx and dres are channel slices [8 : 8 + C) of wider NHWC tensors with
    five different row strides; every result has the bits of the dense run, and nothing outside the slices is written."""
    P, C, _ = br.LD_CASE
    S = br.LD_CASE_STRIDES
    dt = BF if bf16 else torch.float32
    x = br.stats_data(P, C, 30, bf16); dy = br.grad_data(P, C, 31, bf16)
    w, b, mean, invstd, scale, shift = br.bwd_consts(x, C, 32)
    wd, md, isd, scd, shd = (_to(a, dev) for a in (w, mean, invstd, scale, shift))

    def wide(ld, a=None):
        t = torch.full((P, ld), float('nan'), dtype=dt, device=dev)
        if a is not None:
            t[:, 8:8 + C] = _to(a, dev, bf16)
        return t, t[:, 8:]

    def inside(base):                                    # the slice's values; everything around it must still be NaN
        outer = torch.cat([base[:, :8], base[:, 8 + C:]], dim=1)
        assert torch.isnan(outer).all().item(), 'written outside the channel slice'
        return _np(base[:, 8:8 + C])

    outs = []
    for dense in (True, False):
        ws = abi.ws(P, C)
        if dense:
            xd, dyd = _to(x, dev, bf16), _to(dy, dev, bf16)
            lx = ly = ldy_ = C
            y_out = dx_out = dres_out = None
        else:
            (_, xd), (_, dyd) = wide(S['x'], x), wide(S['dy'], dy)
            lx, ly, ldy_ = S['x'], S['y'], S['dy']
            y_out, dx_out, dres_out = wide(S['y']), wide(S['dx']), wide(S['dres'])
        sums = abi.stats(xd, P, C, lx, bf16, ws)
        ws.fill()
        fused = abi.stats_finalize(xd, P, C, lx, bf16, ws, wd, None, 1e-5, 0.1, 0, None, None)
        got = [_np(sums), _np(fused)]
        if not bf16:
            csum = torch.full((C,), float('nan'), device=dev)
            ws.fill()
            abi.call('ssg_channel_sum_f32', abi.lib.ptr(xd), P, C, lx, abi.lib.ptr(csum), ws.ptr())
            got.append(_np(csum))
        y = abi.apply(xd, P, C, lx, scd, shd, dyd, ldy_, ACT_RELU, 0.0, bf16, out=None if dense else (y_out[1], ly))
        ws.fill()
        bs = abi.bwd_reduce(xd, y, dyd, P, C, lx, md, isd, scd, shd, ACT_RELU, 0.0, bf16, ws, with_count=1, lds=(lx, ly, ldy_))
        dx, dres, dwt, dbs = abi.bwd_apply(xd, y, dyd, P, C, lx, md, isd, wd, scd, shd, bs, P, ACT_RELU, 0.0, bf16, lds=(lx, ly, ldy_),
                                           outs=None if dense else ((dx_out[1], S['dx']), (dres_out[1], S['dres'])))
        if dense:
            got += [_np(y), _np(dx), _np(dres)]
        else:
            got += [inside(y_out[0]), inside(dx_out[0]), inside(dres_out[0])]
        outs.append(got + [_np(bs), _np(dwt), _np(dbs)])
        assert ws.intact()
    assert len({S[k] for k in S}) == 5 and min(S.values()) >= 8 + C
    for a, bb in zip(*outs):
        assert a.shape == bb.shape and not np.isnan(a).any() and a.tobytes() == bb.tobytes()


# ----------------------------------------------------------------------------- 8. assembled paths
def _rows(t):
    return np.ascontiguousarray(_np(t).transpose(0, 2, 3, 1).reshape(-1, t.shape[1]))


def _nchw(a, n, h, w):
    return torch.from_numpy(np.ascontiguousarray(a.reshape(n, h, w, a.shape[1]).transpose(0, 3, 1, 2)))


ASSEMBLED = [((1, 256, 13, 2521), 'clamp'), ((1, 260, 11, 29), 'two groups'), ((1, 4, 1, 1), 'one pixel'), ((2, 1, 5, 7), 'psi norm')]


@pytest.mark.parametrize('shape,what', ASSEMBLED, ids=[a[1] for a in ASSEMBLED])
@pytest.mark.parametrize('fused', [True, False], ids=['fused', 'two-launch'])
def test_assembled_f32(pkg, dev, monkeypatch, shape, what, fused):
    ops = pkg.ops
    monkeypatch.setattr(ops, 'BN_FUSED_FINALIZE', fused)
    n, c, h, w_ = shape
    P = n * h * w_
    x = br.stats_data(P, c, 40); dy = br.grad_data(P, c, 41); res = br.grad_data(P, c, 42)
    wt, bs = br.affine_data(c, 43)
    worst = {}
    plans = ((ACT_RELU, True, 1e-5), (ACT_LRELU, False, 1e-3), (ACT_NONE, False, 1e-5))
    for act, with_res, eps in plans[:1 if what == 'clamp' else 3]:              # the 34-MB shape runs one plan: the geometry is what it is for
        bn = torch.nn.BatchNorm2d(c, eps=eps, momentum=0.01).to(dev)
        with torch.no_grad():
            bn.weight.copy_(_to(wt, dev)); bn.bias.copy_(_to(bs, dev))
        xd = _nchw(x, n, h, w_).to(dev).requires_grad_(True)
        rd = _nchw(res, n, h, w_).to(dev).requires_grad_(True) if with_res else None
        y = ops.batch_norm_act(xd, bn, res=rd, act=act, slope=SLOPE)
        y.backward(_nchw(dy, n, h, w_).to(dev))
        assert bn.num_batches_tracked.item() == 1
        r = br.chain_ratios(x, wt, bs, res if with_res else None, act, SLOPE, eps, 0, _rows(y), dy, _rows(xd.grad),
                            _rows(rd.grad) if with_res else None, _np(bn.weight.grad), _np(bn.bias.grad))
        ref = br.stats_ref(x)
        fin = br.finalize_ref(ref['mean'], ref['var'], P, wt, bs, eps, 0.01, 0, np.zeros(c), np.ones(c))
        rg = br.running_gates(ref, fin, br.sum_rel(P, c), eps, 0, 0.01, np.zeros(c), np.ones(c))
        r['running_mean'] = br.worst_ratio(_np(bn.running_mean) - fin['running_mean'], rg['running_mean'])
        r['running_var'] = br.worst_ratio(_np(bn.running_var) - fin['running_var'], rg['running_var'])
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)
    _report('assembled f32 %s %s' % (what, 'fused' if fused else 'two-launch'), worst)
    assert _ok(worst), worst


ASSEMBLED_BF16 = [((1, 512, 13, 2521), 'clamp'), ((1, 520, 3, 53), 'two groups'), ((1, 8, 1, 1), 'one pixel'), ((2, 24, 5, 7), 'idle lanes')]


@pytest.mark.parametrize('shape,what', ASSEMBLED_BF16, ids=[a[1] for a in ASSEMBLED_BF16])
@pytest.mark.parametrize('fused', [True, False], ids=['fused', 'two-launch'])
def test_assembled_bf16(pkg, dev, monkeypatch, shape, what, fused):
    ops, bf = pkg.ops, pkg.bf16
    monkeypatch.setattr(ops, 'BN_FUSED_FINALIZE', fused)
    n, c, h, w_ = shape
    P = n * h * w_
    x = br.stats_data(P, c, 50, True); dy = br.grad_data(P, c, 51, True); res = br.grad_data(P, c, 52, True)
    wt, bs = br.affine_data(c, 53)
    worst = {}
    plans = ((ACT_SWISH, False), (ACT_NONE, True))
    for act, with_res in plans[:1 if what == 'clamp' else 2]:
        bn = torch.nn.BatchNorm2d(c, eps=1e-3, momentum=0.01).to(dev)
        with torch.no_grad():
            bn.weight.copy_(_to(wt, dev)); bn.bias.copy_(_to(bs, dev))
        cl = lambda a: _nchw(a, n, h, w_).to(dev).to(BF).contiguous(memory_format=torch.channels_last)
        xd = cl(x).requires_grad_(True)
        rd = cl(res).requires_grad_(True) if with_res else None
        y = bf.batch_norm_act(xd, bn, res=rd, act=act)
        y.backward(cl(dy))
        assert bn.num_batches_tracked.item() == 1 and y.dtype == BF and xd.grad.dtype == BF
        r = br.chain_ratios(x, wt, bs, res if with_res else None, act, 0.0, 1e-3, 0, _rows(y), dy, _rows(xd.grad),
                            _rows(rd.grad) if with_res else None, _np(bn.weight.grad), _np(bn.bias.grad), bf16=True)
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)
    _report('assembled bf16 %s %s' % (what, 'fused' if fused else 'two-launch'), worst)
    assert _ok(worst), worst
