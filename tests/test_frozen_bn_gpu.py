"""ssg_bn_frozen_bwd_f32 and ssg_bn_fold_bwd_f32 (csrc/bn.hip) through the C-ABI, and ops.batch_norm_act in eval mode through autograd,
against tests/frozen_bn_ref.py.  tests/test_frozen_bn_ref.py rehearses every gate used here on the CPU at these very cases.

Kernel 1, per reduction geometry of bn_ref.STAT_CASES_F32 (TQ / PR / parts edges, P < PR, capped parts, ragged last groups), the
channel-slice case with five distinct strides and the mask probe; per activation NONE / RELU / LRELU 0.2 / SWISH, with y given (a
forward WITH residual, so its mask is not x's) or NULL, dres given or NULL, and the x = mean = scale = NULL form:
* sums bit-identical to ssg_bn_bwd_reduce_f32 on the same inputs (the parent's kernel is the reference of the reduction);
* dres = the fp32 masked gradient, bit for bit (LeakyReLU's dy * slope is the same single fp32 product);
* dx within one fp32 rounding of g * scale in fp64 (two against dy slope scale on LeakyReLU's negative side);
* the recomputed mask equals the forward's y > 0 for pre-activations within rounding of zero, bit for bit;
* two runs give the same bits; the workspace is used at exactly the queried size (NaN-filled, guard band intact);
* bad arguments return a status.
Every geometry runs the whole matrix, the two >= 2^22-element ones included; results that must not depend on an argument (y for NONE
and swish, dres = NULL, a second run) are compared on the device, so the host forms six fp64 references per geometry.

Kernel 2 at (Cout, K) in frozen_bn_ref.FOLD_CASES: dw exact, dgamma / dbeta within one fp32 rounding of the extended-precision
formula plus 2^-50 invstd (sum |dwf w| + |mean sum_g|); NULL outputs honoured.

Assembled: y bit-identical to the no_grad call, dx / dres / dweight / dbias against fp64 torch.nn.functional.batch_norm(training=False).

Worst error / gate measured on an MI355X (pass: <= 1): kernel 1 dres exact, dx 1.00 (a single rounding of a known value meets its
half-ulp bound at 1.00), sums bit-identical (s1 3e-4, s2 0.02 of the fp64 gate), swish dres 0.50, dx 0.54, sums 0.30; kernel 2 dw exact, dgamma 0.94, dbeta 0.98; assembled dx 0.95, dres 0.95, dweight 0.97,
dbias 0.995.  The file's 72 cases take 16 s, the two geometries of 2^22 elements and more 5.0 and 4.4 s of it (six fp64
references each on the host); swish with a residual raises in either mode and is asserted to.
"""
import ctypes as C_

import numpy as np
import pytest
import torch

import bn_ref as br
import frozen_bn_ref as fr
from bn_ref import ACT_LRELU, ACT_NONE, ACT_RELU, ACT_SWISH, F32, F64, U32, f32

pytestmark = pytest.mark.gpu

GUARD = 512
POISON = 0xA5
NAN = float('nan')


def _np(t):
    return np.ascontiguousarray(t.detach().cpu().numpy())


def _to(a, dev):
    return torch.from_numpy(np.array(a, order='C')).to(dev)


def _ok(r):
    return all(v <= 1.0 for v in r.values())


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


class _Ws(object):
    def __init__(self, nbytes, dev):
        self.n = int(nbytes)
        self.buf = torch.empty(self.n + GUARD, dtype=torch.uint8, device=dev)
        assert self.n % 8 == 0 and self.buf.data_ptr() % 16 == 0
        self.fill()

    def fill(self):
        self.buf[:self.n].view(torch.float64).fill_(NAN)
        self.buf[self.n:] = POISON

    def ptr(self):
        return C_.c_void_p(self.buf.data_ptr())

    def intact(self):
        return bool((self.buf[self.n:] == POISON).all().item())


class _Abi(object):
    def __init__(self, pkg, dev):
        self.lib, self.dev = pkg._lib, dev

    def ws(self, P, C):
        return _Ws(self.lib.call('ssg_bn_workspace_bytes', P, C), self.dev)

    def apply(self, x, P, C, scale, shift, res, act, slope):
        p = self.lib.ptr
        y = torch.full((P, C), NAN, device=self.dev)
        self.lib.call('ssg_bn_apply_f32', p(x), P, C, C, p(scale), p(shift), p(res), C if res is not None else 0, act, slope, p(y), C, self.lib.stream_ptr())
        return y

    def bwd_reduce(self, x, y, dy, P, C, mean, invstd, scale, shift, act, slope, ws, lds=None):
        p = self.lib.ptr
        ldx, ldy, lddy = lds or (C, C, C)
        sums = torch.full((2 * C + 1,), NAN, dtype=torch.float64, device=self.dev)
        self.lib.call('ssg_bn_bwd_reduce_f32', p(x), p(y), p(dy), P, C, ldx, ldy if y is not None else 0, lddy, p(mean), p(invstd), p(scale), p(shift),
                      act, slope, p(sums), 0, ws.ptr(), self.lib.stream_ptr())
        return sums[:2 * C]

    def frozen(self, x, y, dy, P, C, mean, invstd, scale, shift, act, slope, ws, want_dx=True, want_dres=True, lds=None, outs=None):
        p = self.lib.ptr
        ldx, ldy, lddy = lds or (C, C, C)
        fresh = lambda want: (torch.full((P, C), NAN, device=self.dev), C) if want else (None, 0)
        (dx, lddx), (dres, lddres) = outs if outs is not None else (fresh(want_dx), fresh(want_dres))
        sums = torch.full((2 * C,), NAN, dtype=torch.float64, device=self.dev)
        self.lib.call('ssg_bn_frozen_bwd_f32', p(x), p(y), p(dy), P, C, ldx if x is not None else 0, ldy if y is not None else 0, lddy,
                      p(mean), p(invstd), p(scale), p(shift), act, slope, p(dx), lddx, p(dres), lddres, p(sums), ws.ptr(), self.lib.stream_ptr())
        return dx, dres, sums


@pytest.fixture()
def abi(pkg, dev):
    return _Abi(pkg, dev)


def _case(P, C, seed):
    mean, invstd, w, b, scale, shift = fr.frozen_consts(C, seed)
    x = fr.frozen_x(P, C, mean, invstd, seed + 1)
    dy = br.grad_data(P, C, seed + 2)
    res = f32(np.random.RandomState(seed + 3).standard_normal((P, C)) * 2.0)
    return x, dy, res, mean, invstd, scale, shift


# ----------------------------------------------------------------------------- kernel 1
def _matrix(abi, dev, P, C, seed, strides=None):
    """The whole matrix at one geometry: act in {NONE, RELU, LRELU 0.2, SWISH} x (y NULL | y given) x (dres given | NULL), and the
    x = mean = scale = NULL form; every output gated on the host, the sums compared with ssg_bn_bwd_reduce_f32 bit for bit.
    `strides`: dict(x, y, dy, dx, dres) -- every tensor is then the channel slice [8 : 8 + C) of a wider row with its own stride, and
    nothing outside the output slices may be written.  Returns (worst ratios, every output in call order)."""
    x, dy, res, mean, invstd, scale, shift = _case(P, C, seed)
    xd, dyd, resd, md, isd, scd, shd = (_to(a, dev) for a in (x, dy, res, mean, invstd, scale, shift))
    ws = abi.ws(P, C)
    S = strides

    def wide(ld, t=None):
        base = torch.full((P, ld), NAN, device=dev)
        if t is not None:
            base[:, 8:8 + C] = t
        return base

    def inside(base):
        assert torch.isnan(torch.cat([base[:, :8], base[:, 8 + C:]], dim=1)).all().item(), 'written outside the channel slice'
        return base[:, 8:8 + C].contiguous()

    xs = wide(S['x'], xd)[:, 8:] if S else xd
    dys = wide(S['dy'], dyd)[:, 8:] if S else dyd

    def run(xin, y, act, slope, consts=True, want_dx=True, want_dres=True):
        ws.fill()
        m, i, sc, sh = (md, isd, scd, shd) if consts else (None, None, None, None)
        if not S:
            return abi.frozen(xin, y, dyd, P, C, m, i, sc, sh, act, slope, ws, want_dx=want_dx, want_dres=want_dres)
        ys = wide(S['y'], y)[:, 8:] if y is not None else None
        dxw = wide(S['dx']) if want_dx else None
        drw = wide(S['dres']) if want_dres else None
        _, _, sums = abi.frozen(xs if xin is not None else None, ys, dys, P, C, m, i, sc, sh, act, slope, ws, lds=(S['x'], S['y'], S['dy']),
                                outs=((dxw[:, 8:], S['dx']) if want_dx else (None, 0), (drw[:, 8:], S['dres']) if want_dres else (None, 0)))
        return (inside(dxw) if want_dx else None), (inside(drw) if want_dres else None), sums

    def reduce(y, act, slope):
        ws.fill()
        if not S:
            return abi.bwd_reduce(xd, y, dyd, P, C, md, isd, scd, shd, act, slope, ws)
        ys = wide(S['y'], y)[:, 8:] if y is not None else None
        return abi.bwd_reduce(xs, ys, dys, P, C, md, isd, scd, shd, act, slope, ws, lds=(S['x'], S['y'], S['dy']))

    f32v = lambda t: t.view(torch.float32)
    worst, outs = {}, []
    for act in fr.ACTS:
        slope = fr.slope_of(act)
        masked = act in (ACT_RELU, ACT_LRELU)
        y_plain = abi.apply(xd, P, C, scd, shd, None, act, slope)
        # y = NULL: the mask is recomputed, = the plain forward's.  y given: a forward WITH residual (its mask is not x's) where the
        # activation reads y; elsewhere y is ignored and the result must not change
        plans = [(None, y_plain), ((abi.apply(xd, P, C, scd, shd, resd, act, slope),) * 2 if masked else (y_plain, y_plain))]
        first = None
        for y, y_fwd in plans:
            dx, dres, sums = run(xd, y, act, slope)
            assert _bits(f32v(sums), f32v(reduce(y, act, slope))), 'sums differ from ssg_bn_bwd_reduce_f32 (act %d)' % act
            if masked or first is None:
                r = fr.frozen_ratios(x, _np(y_fwd) > 0, dy, mean, invstd, scale, shift, act, slope, dx=_np(dx), dres=_np(dres), s1=_np(sums[:C]),
                                     s2=_np(sums[C:]))
                for k, v in r.items():
                    k = ('swish_' + k) if act == ACT_SWISH else k
                    worst[k] = max(worst.get(k, 0.0), v)
            else:
                assert _bits(dx, first[0]) and _bits(dres, first[1]) and _bits(f32v(sums), f32v(first[2])), 'y changed the result of an activation that does not read it'
            first = first or (dx, dres, sums)
            dx2, dres2, sums2 = run(xd, y, act, slope)                                    # the same call again: the same bits
            assert _bits(dx, dx2) and _bits(dres, dres2) and _bits(f32v(sums), f32v(sums2)), 'two runs differ'
            dx3, none, sums3 = run(xd, y, act, slope, want_dres=False)                   # dres = NULL
            assert none is None and _bits(dx, dx3) and _bits(f32v(sums), f32v(sums3))
            outs += [dx, dres, f32v(sums)]
            if act != ACT_SWISH and (y is not None or act == ACT_NONE):
                # activation backward + bias gradient: x = mean = scale = NULL; dx = g, first half of the sums the same bits, second 0
                gx, gres, gs = run(None, y if masked else None, act, slope, consts=False)
                assert _bits(gx, dres) and _bits(gres, dres) and _bits(f32v(gs[:C]), f32v(sums[:C])) and not gs[C:].any().item()
                gx2, none, gs2 = run(None, y if masked else None, act, slope, consts=False, want_dres=False)
                assert none is None and _bits(gx2, gx) and _bits(f32v(gs2), f32v(gs))
                outs += [gx, f32v(gs)]
    assert ws.intact()
    return worst, outs


@pytest.mark.parametrize('case', br.STAT_CASES_F32, ids=lambda c: '%dx%d' % c[:2])
def test_frozen_bwd(abi, dev, case):
    P, C = case[:2]
    assert not br.check_facts(P, C, 1, case[2])
    worst, _ = _matrix(abi, dev, P, C, 100 + C)
    print('RATIO frozen_bwd %dx%d %s' % (P, C, '  '.join('%s=%.3g' % kv for kv in sorted(worst.items()))))
    assert _ok(worst), worst


def test_channel_slices_with_distinct_strides(abi, dev):
    """The same matrix with x, y, dy, dx, dres as channel slices [8 : 8 + C) of wider rows, five different strides: every gate again,
    the bits of the dense run, and nothing outside the slices written."""
    P, C, _ = br.LD_CASE
    S = br.LD_CASE_STRIDES
    assert len(set(S.values())) == 5 and min(S.values()) >= 8 + C
    worst_d, dense = _matrix(abi, dev, P, C, 30)
    worst_s, wide = _matrix(abi, dev, P, C, 30, strides=S)
    assert _ok(worst_d) and _ok(worst_s), (worst_d, worst_s)
    assert len(dense) == len(wide) and all(_bits(a, b) for a, b in zip(dense, wide))


def test_swish_needs_x_and_bad_arguments_return_a_status(abi, dev):
    P, C = 8, 8
    z = torch.zeros((P, C), device=dev); v = torch.ones(C, device=dev)
    ws = abi.ws(P, C)
    E = abi.lib.HipLibraryError
    with pytest.raises(E):                                   # swish without x
        abi.frozen(None, z, z, P, C, None, None, v, v, ACT_SWISH, 0.0, ws)
    with pytest.raises(E):                                   # a mask activation with neither y nor (x, scale, shift)
        abi.frozen(None, None, z, P, C, None, None, None, None, ACT_RELU, 0.0, ws)
    with pytest.raises(E):                                   # C % 4
        abi.frozen(z, None, z, P, 6, v, v, v, v, ACT_NONE, 0.0, ws, lds=(8, 8, 8), outs=((z.clone(), 8), (None, 0)))
    with pytest.raises(E):                                   # mean without x
        abi.frozen(None, None, z, P, C, v, v, None, None, ACT_NONE, 0.0, ws)
    odd = torch.zeros(P * C + 4, device=dev)[1:1 + P * C].view(P, C)                       # 4 bytes off a 16-byte boundary
    assert odd.data_ptr() % 16 != 0
    for kw in (dict(x=odd), dict(dy=odd), dict(dx=odd)):
        with pytest.raises(E):
            abi.frozen(kw.get('x', z), None, kw.get('dy', z), P, C, v, v, v, v, ACT_NONE, 0.0, ws, outs=((kw.get('dx', z.clone()), C), (None, 0)))
    assert ws.intact()


@pytest.mark.parametrize('act', [ACT_RELU, ACT_LRELU])
def test_recomputed_mask_is_the_forward_mask(abi, dev, act):
    C, P = 2048, 18
    x, scale, shift = br.mask_probe(C, P, 21)
    slope = fr.slope_of(act)
    xd, scd, shd = _to(x, dev), _to(scale, dev), _to(shift, dev)
    y = abi.apply(xd, P, C, scd, shd, None, act, slope)
    pos = _np(y) > 0
    assert pos.any() and (~pos).any()
    dy = torch.ones((P, C), device=dev)
    want = np.where(pos, F32(1), F32(0) if act == ACT_RELU else F32(slope))
    ws = abi.ws(P, C)
    got = []
    for yy in (None, y):
        _, dres, sums = abi.frozen(xd, yy, dy, P, C, None, None, scd, shd, act, slope, ws, want_dx=False)
        n_bad = int((_np(dres) != want).sum())
        assert n_bad == 0, '%d of %d masks differ from y > 0' % (n_bad, P * C)
        got.append((dres, sums))
    assert _bits(got[0][0], got[1][0]) and _bits(got[0][1].view(torch.float32), got[1][1].view(torch.float32))
    assert ws.intact()


# ----------------------------------------------------------------------------- kernel 2
@pytest.mark.parametrize('Cout,K', fr.FOLD_CASES)
def test_fold_bwd(pkg, dev, Cout, K):
    lib = pkg._lib
    p = lib.ptr
    data = fr.fold_data(Cout, K, 50 + Cout)
    dwf, w, s, mean, invstd, sums_g = (_to(a, dev) for a in data)

    def run(want_w, want_gb):
        dw = torch.full((Cout, K), NAN, device=dev) if want_w else None
        dgb = torch.full((2, Cout + 8), NAN, device=dev)
        lib.call('ssg_bn_fold_bwd_f32', p(dwf), p(w), Cout, K, p(s), p(mean), p(invstd), p(sums_g), p(dw),
                 p(dgb[0]) if want_gb else None, p(dgb[1]) if want_gb else None, lib.stream_ptr())
        assert torch.isnan(dgb[:, Cout:]).all().item()
        if not want_gb:
            assert torch.isnan(dgb).all().item()
        return dw, dgb[0, :Cout], dgb[1, :Cout]

    dw, dg, db = run(True, True)
    r = fr.fold_ratios(*data, dw=_np(dw), dgamma=_np(dg), dbeta=_np(db))
    print('RATIO fold_bwd %dx%d %s' % (Cout, K, '  '.join('%s=%.3g' % kv for kv in sorted(r.items()))))
    assert _ok(r) and r['dw'] == 0.0, r
    dw2, _, _ = run(True, False)
    none, dg3, db3 = run(False, True)
    assert none is None and _bits(dw, dw2) and _bits(dg, dg3) and _bits(db, db3)
    with pytest.raises(lib.HipLibraryError):
        lib.call('ssg_bn_fold_bwd_f32', p(dwf), p(w), Cout, K, p(s), p(mean), p(invstd), p(sums_g), None, None, None, lib.stream_ptr())
    with pytest.raises(lib.HipLibraryError):
        lib.call('ssg_bn_fold_bwd_f32', p(dwf), None, Cout, K, p(s), p(mean), p(invstd), p(sums_g), None, p(dg), p(db), lib.stream_ptr())


# ----------------------------------------------------------------------------- assembled: ops.batch_norm_act in eval mode
def _rows(t, c=None):
    a = _np(t)
    return np.ascontiguousarray(a.transpose(0, 2, 3, 1).reshape(-1, a.shape[1]))


# swish with a residual is unsupported in either mode (its derivative needs the pre-activation sum, which nobody keeps): it raises
ACT_RES = [(a, r) for a in fr.ACTS for r in (False, True) if not (a == ACT_SWISH and r)]


def test_batch_norm_act_eval_swish_with_residual_raises(pkg, dev):
    bn = torch.nn.BatchNorm2d(8).to(dev).eval()
    x = torch.randn(2, 8, 5, 3, device=dev)
    with pytest.raises(NotImplementedError):
        pkg.ops.batch_norm_act(x.clone().requires_grad_(True), bn, res=x, act=ACT_SWISH)
    with torch.no_grad(), pytest.raises(pkg._lib.HipLibraryError):                     # the kernel itself refuses it in any forward
        pkg.ops.batch_norm_act(x, bn, res=x, act=ACT_SWISH)


@pytest.mark.parametrize('shape', fr.ASSEMBLED, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('act,with_res', ACT_RES)
def test_batch_norm_act_eval_backward(pkg, dev, shape, act, with_res):
    ops = pkg.ops
    n, c, h, w = shape
    slope = fr.slope_of(act)
    mean, invstd0, wt, bs, _, _ = fr.frozen_consts(c, 60 + c)
    bn = torch.nn.BatchNorm2d(c).to(dev)
    with torch.no_grad():
        bn.weight.copy_(_to(wt, dev)); bn.bias.copy_(_to(bs, dev)); bn.running_mean.copy_(_to(mean, dev))
        bn.running_var.copy_(_to(f32(1.0 / invstd0.astype(F64) ** 2), dev))
    bn.eval()
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    rng = np.random.RandomState(70 + c)
    nchw = lambda a: torch.from_numpy(f32(a)).permute(0, 3, 1, 2)
    x = nchw(mean.astype(F64) + rng.standard_normal((n, h, w, c)) / invstd0.astype(F64))
    res = nchw(rng.standard_normal((n, h, w, c)) * 2) if with_res else None
    up = nchw(rng.standard_normal((n, h, w, c)))
    xd = x.to(dev).requires_grad_(True)
    rd = res.to(dev).requires_grad_(True) if with_res else None
    with torch.no_grad():
        y0 = ops.batch_norm_act(xd, bn, res=rd, act=act, slope=slope)
    y = ops.batch_norm_act(xd, bn, res=rd, act=act, slope=slope)
    assert _bits(y0.contiguous(), y.contiguous()), 'recorded forward differs from the no_grad forward'
    y.backward(up.to(dev))
    assert _bits(bn.running_mean, rm0) and _bits(bn.running_var, rv0) and bn.num_batches_tracked.item() == 0
    # the layer's own fp32 constants, formed with its torch ops on the device
    with torch.no_grad():
        isd = torch.rsqrt(bn.running_var + bn.eps); scd = isd * bn.weight; shd = -bn.running_mean * scd + bn.bias
    isf, scale, shift = _np(isd), _np(scd), _np(shd)
    # fp64 reference on the CPU: F.batch_norm(training=False) at the variance whose rsqrt(var + eps) is that fp32 invstd, the activation
    # pattern of the HIP forward imposed (as tests/test_grad_parity_gpu.py does)
    pos = y.detach().cpu() > 0
    x64 = x.double().requires_grad_(True)
    r64 = res.double().requires_grad_(True) if with_res else None
    w64 = torch.from_numpy(wt).double().requires_grad_(True); b64 = torch.from_numpy(bs).double().requires_grad_(True)
    var64 = 1.0 / torch.from_numpy(isf).double() ** 2 - bn.eps
    z = torch.nn.functional.batch_norm(x64, torch.from_numpy(mean).double(), var64, w64, b64, False, 0.0, bn.eps)
    if with_res:
        z = z + r64
    if act == ACT_SWISH:
        out = z * torch.sigmoid(z)
    elif act == ACT_NONE:
        out = z
    else:
        out = torch.where(pos, z, z * (0.0 if act == ACT_RELU else float(F32(slope))))
    out.backward(up.double())
    ref = dict(dx=_rows(x64.grad), dweight=w64.grad.numpy(), dbias=b64.grad.numpy())
    got = dict(dx=_rows(xd.grad), dweight=_np(bn.weight.grad), dbias=_np(bn.bias.grad))
    assert got['dweight'].shape == (c,) and got['dbias'].shape == (c,) and tuple(xd.grad.shape) == shape
    if with_res:
        ref['dres'] = _rows(r64.grad); got['dres'] = _rows(rd.grad)
    r = fr.assembled_ratios(_rows(x), _rows(pos.float()) > 0, _rows(up), mean, isf, scale, shift, act, slope, ref, got)
    print('RATIO eval bn %s act %d res %d %s' % (shape, act, with_res, '  '.join('%s=%.3g' % kv for kv in sorted(r.items()))))
    assert _ok(r), r


def test_batch_norm_act_eval_without_affine_and_without_grad(pkg, dev):
    """affine=False: no parameter gradients, dx = g invstd; requires_grad off everywhere: nothing is recorded."""
    ops = pkg.ops
    bn = torch.nn.BatchNorm2d(8, affine=False).to(dev)
    with torch.no_grad():
        bn.running_mean.normal_(); bn.running_var.uniform_(0.5, 2.0)
    bn.eval()
    x = torch.randn(2, 8, 5, 3, device=dev)
    y = ops.batch_norm_act(x, bn, act=ACT_RELU)
    assert not y.requires_grad
    xg = x.clone().requires_grad_(True)
    y = ops.batch_norm_act(xg, bn, act=ACT_RELU)
    y.backward(torch.ones_like(y))
    want = torch.where(y.detach() > 0, torch.rsqrt(bn.running_var + bn.eps).view(1, -1, 1, 1).expand_as(y), torch.zeros_like(y))
    assert _bits(xg.grad.contiguous(), want.contiguous())
