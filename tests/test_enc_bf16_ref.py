"""CPU rehearsal of tests/enc_bf16_ref.py, the reference module of tests/test_enc_bf16_gpu.py (the bf16 encoder kernels: GEMM,
stem conv, converts).  The table's literals against the built library's host queries; the fp64 references against fp64 torch;
the integer class exact at every case; the clean emulation through every gate at every case; each planted defect failing the
gate meant for it at a named case; the host refusals of every entry point (fake aligned pointers that are never dereferenced:
every argument set here is rejected before any launch); check_coverage()."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import enc_bf16_ref as er
from enc_bf16_ref import F32, F64, f32

GEMM = {c.name: c for c in er.GEMM_CASES}
WG = {c.name: c for c in er.WG_CASES}
STEM = {c.name: c for c in er.ALL_TABLES['stem']}


# ----------------------------------------------------------------------------- bf16_rne
def test_bf16_rne_is_bit_exact():
    v = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -23, 257.0, 259.0, -257.0, 3.4e38, -3.4e38, 3.39e38,
                  np.inf, -np.inf, 0.0, -0.0], dtype=F32)
    want = np.array([1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, 256.0, 260.0, -256.0, np.inf, -np.inf, 3.3895314e38, np.inf, -np.inf, 0.0, -0.0], dtype=F32)
    assert er.first_mismatch(er.bf16_rne(v), want) is None, er.first_mismatch(er.bf16_rne(v), want)
    nans = np.array([0x7FC00000, 0x7F800001, 0x7FFFFFFF, 0xFFFFFFFF, 0xFF800001], dtype=np.uint32).view(F32)
    assert np.isnan(er.bf16_rne(nans)).all()
    # against torch's conversion over random bits of every exponent
    rng = np.random.RandomState(5)
    bits = rng.randint(0, 2 ** 32, 200000, dtype=np.uint64).astype(np.uint32)
    a = bits.view(F32)
    t = torch.from_numpy(a.copy()).to(torch.bfloat16).float().numpy()
    assert er.same_bits(er.bf16_rne(a), t)
    assert er.is_bf16(er.bf16_rne(a)) and not er.is_bf16(np.array([1.0 + 2.0 ** -9], dtype=F32))


# ----------------------------------------------------------------------------- literals against the library's host queries
def test_literals_match_the_library(pkg):
    call = pkg._lib.call
    for c in er.WG_CASES:
        nbytes = call('ssg_gemm_wgrad_bf16_workspace_bytes', c.P, c.M, c.N)
        assert nbytes == c.ws_bytes and nbytes // (4 * c.M * c.N) == c.splits and nbytes % (4 * c.M * c.N) == 0, (c.name, nbytes)
        assert er.wg_plan(c.P, c.M, c.N) == (c.splits, c.sps, c.empty, c.reducer, c.ws_bytes), c.name
    for c in er.ALL_TABLES['stem']:
        assert call('ssg_conv2d_thin_bf16_wgrad_workspace_bytes', c.N, c.OH, c.OW, c.Cout, c.KH, c.KW) == c.ws_bytes, c.name
    assert call('ssg_conv2d_thin_bf16_wgrad_workspace_bytes', 0, 4, 4, 8, 3, 3) == 0
    # the split rule over a sweep, restated rule against the library
    for P in (1, 255, 256, 257, 8191, 8192, 70000, 10 ** 6, 4 * 512 * 512):
        for M, N in ((8, 8), (24, 144), (128, 128), (136, 264), (448, 2688), (112, 672)):
            assert call('ssg_gemm_wgrad_bf16_workspace_bytes', P, M, N) == er.wg_plan(P, M, N)[4], (P, M, N)


def test_check_coverage():
    assert er.check_coverage() == len(er.GEMM_CASES) + len(er.WG_CASES) + len(er.STEM_CASES) + 1 + len(er.ROWS_CASES)
    assert all(len(v) > 20 for v in er.LEFT_OUT.values())


# ----------------------------------------------------------------------------- references against fp64 torch
def test_gemm_and_pack_references_against_torch():
    c = GEMM['t12_k136_n136_t']
    x, W, res = er.gemm_rand_data(c)
    we = er.w_eff(c, W)
    ref = er.gemm_ref(x, we, res)
    t = torch.from_numpy(x).double() @ torch.from_numpy(W).double() + torch.from_numpy(res).double()      # W is [K][N] here
    assert np.allclose(ref, t.numpy(), rtol=1e-13, atol=1e-13)
    p = er.pack_ref(W, 1, 256, 160)
    assert p.shape == (256, 160) and er.same_bits(p[:c.N, :c.K], we) and not p[c.N:].any() and not p[:, c.K:].any()
    p0 = er.pack_ref(we, 0, 256, 160)
    assert er.same_bits(p, p0) and er.same_bits(er.pack_emul(W, 1, 256, 160), p)
    w = WG['p4133_24x264']
    dy, xx = er.wg_rand_data(w)
    assert np.allclose(er.gemm_wgrad_ref(dy, xx), (torch.from_numpy(dy).double().t() @ torch.from_numpy(xx).double()).numpy(), rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize('name', ['k3c32_s2_same', 'k5c40_s2_p1212', 'k1x3c8', 'ow1_s2', 'k3c64_s1', 'k1c8_cin1'])
def test_stem_references_against_torch(name):
    c = STEM[name]
    x, w, dy = er.stem_rand_data(c)
    pt, pb, pl, pr = c.pads
    xt = torch.from_numpy(er.bf16_rne(x)).double().permute(0, 3, 1, 2).requires_grad_(True)
    wt = torch.from_numpy(er.bf16_rne(w)).double().requires_grad_(True)
    y = F.conv2d(F.pad(xt, (pl, pr, pt, pb)), wt, None, c.stride)
    assert tuple(y.shape) == (c.N, c.Cout, c.OH, c.OW)
    y.backward(torch.from_numpy(dy).double().permute(0, 3, 1, 2))
    assert np.allclose(er.stem_fwd_ref(x, w, c.stride, pt, pl, c.OH, c.OW), y.detach().permute(0, 2, 3, 1).numpy(), rtol=1e-12, atol=1e-12)
    assert np.allclose(er.stem_wgrad_ref(x, dy, c.KH, c.KW, c.stride, pt, pl), wt.grad.numpy(), rtol=1e-12, atol=1e-11)
    assert np.allclose(er.stem_dgrad_ref(dy, w, c.H, c.W, c.stride, pt, pl), xt.grad.permute(0, 2, 3, 1).numpy(), rtol=1e-12, atol=1e-12)


def test_stem_forward_emulation_is_the_scalar_fma_chain():
    """stem_fwd_emul (vectorised) against the chain written out pixel by pixel, bit for bit."""
    c = STEM['ow2_s2_same']
    x, w, _ = er.stem_rand_data(c)
    xr = er.bf16_rne(x).astype(F64); wr = er.bf16_rne(w).astype(F64)
    pt, _, pl, _ = c.pads
    want = np.zeros((c.N, c.OH, c.OW, c.Cout), dtype=F32)
    for n in range(c.N):
        for oy in range(c.OH):
            for ox in range(c.OW):
                for co in range(c.Cout):
                    acc = F32(0)
                    for ky in range(c.KH):
                        for kx in range(c.KW):
                            iy, ix = oy * c.stride - pt + ky, ox * c.stride - pl + kx
                            if 0 <= iy < c.H and 0 <= ix < c.W:
                                for ci in range(c.Cin):
                                    acc = F32(F64(acc) + xr[n, iy, ix, ci] * wr[co, ci, ky, kx])
                    want[n, oy, ox, co] = acc
    assert er.same_bits(er.stem_fwd_emul(c, x, w), er.bf16_rne(want))


# ----------------------------------------------------------------------------- the integer class is exact, case by case
@pytest.mark.parametrize('table', ['gemm', 'wgrad', 'stem'])
def test_int_class_is_exact_at_every_case(table):
    ties = 0
    for c in er.ALL_TABLES[table]:
        assert er.int_class_is_exact(c), c.name
        if table == 'gemm':
            x, W, res = er.gemm_int_data(c)
            a, b = er.has_ties(er.gemm_ref(x, er.w_eff(c, W)))
            ties += a and b
    if table == 'gemm':
        assert ties >= 8, ties            # sums above 256 and odd integers in [256, 512) occur: a truncating store cannot pass


# ----------------------------------------------------------------------------- the clean emulation passes every gate
def gemm_run(c, cls, use_res, variant=0, **defects):
    x, W, res = er.gemm_data(c, cls, variant)
    if cls == 1 or not use_res:
        res = None
    we = er.w_eff(c, W)
    rows_pad = er.round_up(c.N, 128)
    wp = er.pack_emul(W, c.transpose, rows_pad, c.Kp, wrong_transpose=defects.pop('wrong_transpose', False))
    if c.nan_rows:
        wp[c.N:] = np.nan
    rb = None if res is None else er.res_buffer(c, res)
    got = er.gemm_emul(c, x, wp, rb, ldo=c.N + 8, **defects)
    ref, mag = er.gemm_ref(x, we, res, mag=True)
    emu = er.gemm_emul(c, x, er.pack_emul(W, c.transpose, rows_pad, c.Kp), rb) if cls == 2 else None
    return er.judge(cls, got, ref, True, er.gemm_gate(c, ref, mag), emu)


@pytest.mark.parametrize('name', sorted(GEMM))
def test_gemm_clean_emulation_passes(name):
    c = GEMM[name]
    for cls in (0, 1, 2):
        for use_res in (False, True):
            for v in ((0, 1) if cls == 1 else (0,)):
                r = gemm_run(c, cls, use_res, v)
                assert er.passes(r), (name, cls, use_res, r)


def wg_run(c, cls, variant=0, reducer=None, **defects):
    dy, x = er.wg_data(c, cls, variant)
    ref, mag = er.gemm_wgrad_ref(dy, x, mag=True)
    got = er.wg_emul(c, dy, x, reducer=reducer, **defects)
    emu = er.wg_emul(c, dy, x) if cls == 2 else None
    return er.judge(cls, got, ref, False, er.wg_gate(c, ref, mag), emu)


@pytest.mark.parametrize('name', sorted(WG))
def test_wgrad_clean_emulation_passes_in_both_reduce_orders(name):
    c = WG[name]
    for cls in (0, 1, 2):
        for red in ((er.REDUCE_SERIAL, er.REDUCE_32) if c.P < 20000 or cls < 2 else (None,)):
            for v in ((0, 1) if cls == 1 else (0,)):
                r = wg_run(c, cls, v, red)
                assert er.passes(r), (name, cls, red, r)


def stem_run(c, cls, op, variant=0, **defects):
    x, w, dy = er.stem_data(c, cls, op, variant)
    pt, _, pl, _ = c.pads
    if op == 'fwd':
        ref, mag = er.stem_fwd_ref(x, w, c.stride, pt, pl, c.OH, c.OW, mag=True)
        got = er.stem_fwd_emul(c, x, w, **defects)
        return er.judge(cls, got, ref, True, er.stem_fwd_gate(c, ref, mag), er.stem_fwd_emul(c, x, w) if cls == 2 else None)
    if op == 'wgrad':
        ref, mag = er.stem_wgrad_ref(x, dy, c.KH, c.KW, c.stride, pt, pl, mag=True)
        got = er.stem_wgrad_emul(c, x, dy, **defects)
        return er.judge(cls, got, ref, False, er.stem_wgrad_gate(c, ref, mag), er.stem_wgrad_emul(c, x, dy) if cls == 2 else None)
    ref, mag = er.stem_dgrad_ref(dy, w, c.H, c.W, c.stride, pt, pl, mag=True)
    got = er.stem_dgrad_emul(c, dy, w, **defects)
    return er.judge(cls, got, ref, False, er.stem_dgrad_gate(c, ref, mag), er.stem_dgrad_emul(c, dy, w) if cls == 2 else None)


@pytest.mark.parametrize('name', sorted(STEM))
def test_stem_clean_emulation_passes(name):
    c = STEM[name]
    for op in ('fwd', 'wgrad', 'dgrad'):
        for cls in (0, 1, 2):
            if ('stem', name, op) in er.EXEMPT and cls == 2:
                continue
            for v in ((0, 1) if cls == 1 else (0,)):
                r = stem_run(c, cls, op, v)
                assert er.passes(r), (name, op, cls, r)


def test_rows_references():
    for c in er.ROWS_CASES:
        a, a_bf, b_bf = er.rows_data(c)
        assert er.is_bf16(a_bf) and er.is_bf16(b_bf)
        s = er.add_ref(a_bf, b_bf)
        t = (torch.from_numpy(a_bf) + torch.from_numpy(b_bf)).to(torch.bfloat16).float().numpy()
        assert er.same_bits(s, t), c.name
        assert np.isnan(s).any() and np.isinf(s).any()
        fin = np.isfinite(s)
        exact = a_bf[fin].astype(F64) + b_bf[fin].astype(F64)
        assert (er.bf16_rne(f32(exact)) != er.bf16_trunc(f32(exact))).any(), c.name            # ties are present
        assert er.same_bits(er.convert_ref(a, True), torch.from_numpy(a).to(torch.bfloat16).float().numpy())


# ----------------------------------------------------------------------------- every planted defect fails the gate meant for it
GEMM_DEFECTS = [   # (defect, case, class, res, variant, gate)
    ('truncate', 't8_k72_n120', 0, False, 0, 'bits'), ('truncate', 't8_k72_n120', 2, True, 0, 'hard'),
    ('half_away', 't9_k96_n128', 0, True, 0, 'bits'),
    ('drop_last_step', 'p129_k40_n136', 0, False, 0, 'bits'), ('drop_last_step', 't12_k136_n136_t', 2, False, 0, 'hard'),
    ('tail_chunk_zero', 'p127_k24_n120', 0, False, 0, 'bits'), ('tail_chunk_zero', 'p127_k48_n8_t', 2, False, 0, 'hard'),
    ('swizzle_off', 't7_k64_n8', 1, False, 0, 'bits'), ('swizzle_off', 'p129_k672_n264_t', 0, False, 0, 'bits'),
    ('res_stride_ldo', 'p129_k40_n136', 0, True, 0, 'bits'), ('res_stride_ldo', 't7_k64_n8', 2, True, 0, 'hard'),
    ('wrong_transpose', 'p127_k48_n8_t', 1, False, 0, 'bits'), ('wrong_transpose', 't12_k136_n136_t', 0, False, 0, 'bits'),
    ('drop_pixel_tail', 'p129_k40_n136', 0, False, 0, 'bits'), ('drop_pixel_tail', 'p1_k8_n8', 2, False, 0, 'hard'),
]


@pytest.mark.parametrize('defect,name,cls,use_res,variant,gate', GEMM_DEFECTS)
def test_gemm_defect_fails_its_gate(defect, name, cls, use_res, variant, gate):
    c = GEMM[name]
    assert er.passes(gemm_run(c, cls, use_res, variant))
    r = gemm_run(c, cls, use_res, variant, **{defect: True})
    assert r[gate] > 1.0, (defect, name, r)


def test_gemm_res_stride_defect_is_invisible_only_at_row_zero():
    """P = 1: the residual's row 0 starts at the same address for every stride, so the case cannot see the defect -- which is why
    the defect is pinned at P = 129 above."""
    c = GEMM['p1_k8_n8']
    assert er.passes(gemm_run(c, 0, True, 0, res_stride_ldo=True))


WG_DEFECTS = [
    ('drop_last_split', 'p4133_8x8', 0, 0, 'bits'), ('drop_last_split', 'p4133_24x264', 1, 1, 'bits'), ('drop_last_split', 'p16400_24x8', 2, 0, 'hard'),
    ('stale_empty', 'p4133_8x8', 0, 0, 'bits'), ('stale_empty', 'p16400_24x8', 2, 0, 'hard'),
    ('drop_pixel_tail', 'p33_24x24', 1, 1, 'bits'), ('drop_pixel_tail', 'p1_8x8', 0, 0, 'bits'),
    ('drop_last_step', 'p255_128x136', 0, 0, 'bits'), ('drop_last_step', 'p512_264x8', 2, 0, 'hard'),
]


@pytest.mark.parametrize('defect,name,cls,variant,gate', WG_DEFECTS)
def test_wgrad_defect_fails_its_gate(defect, name, cls, variant, gate):
    c = WG[name]
    assert er.passes(wg_run(c, cls, variant))
    r = wg_run(c, cls, variant, **{defect: True})
    assert r[gate] > 1.0, (defect, name, r)


STEM_DEFECTS = [   # (defect, op, case, class, variant, gate)
    ('truncate', 'fwd', 'k3c32_s2_same', 0, 0, 'bits'), ('truncate', 'fwd', 'k3c48_s2_sym', 2, 0, 'hard'),
    ('swap_kykx', 'fwd', 'k3c8_s1', 1, 1, 'bits'), ('swap_kykx', 'wgrad', 'k3c8_s1', 0, 0, 'bits'), ('swap_kykx', 'dgrad', 'k3c8_s1', 0, 0, 'bits'),
    ('pad_wrong_side', 'fwd', 'k3c32_s2_same', 0, 0, 'bits'), ('pad_wrong_side', 'wgrad', 'ow2_s2_same', 1, 0, 'bits'),
    ('pad_wrong_side', 'fwd', 'k5c40_s2_p1212', 2, 0, 'hard'),
    ('x_unrounded', 'fwd', 'k3c32_s2_same', 2, 0, 'hard'), ('x_unrounded', 'wgrad', 'k3c32_s2_same', 2, 0, 'hard'),
    ('wrap_early', 'wgrad', 'ow2_s2_same', 0, 0, 'bits'), ('wrap_early', 'wgrad', 'k3c64_s1', 1, 1, 'bits'), ('wrap_early', 'wgrad', 'k1c8_cin1', 2, 0, 'hard'),
    ('stop_after_64', 'wgrad', 'b72_s2_same', 0, 0, 'bits'), ('stop_after_64', 'wgrad', 'b72_s2_same', 1, 1, 'bits'),
    ('ignore_parity', 'dgrad', 'k3c32_s2_same', 0, 0, 'bits'), ('ignore_parity', 'dgrad', 'k5c40_s2_p1212', 1, 0, 'bits'),
]


@pytest.mark.parametrize('defect,op,name,cls,variant,gate', STEM_DEFECTS)
def test_stem_defect_fails_its_gate(defect, op, name, cls, variant, gate):
    c = STEM[name]
    assert er.passes(stem_run(c, cls, op, variant))
    r = stem_run(c, cls, op, variant, **{defect: True})
    assert r[gate] > 1.0, (defect, op, name, r)


def test_no_defect_is_left_without_a_failing_gate():
    import inspect
    planted = set()
    for fn in (er.gemm_emul, er.wg_emul, er.stem_fwd_emul, er.stem_wgrad_emul, er.stem_dgrad_emul, er.pack_emul):
        planted |= {k for k, p in inspect.signature(fn).parameters.items() if p.default is False}
    shown = {d[0] for d in GEMM_DEFECTS} | {d[0] for d in WG_DEFECTS} | {d[0] for d in STEM_DEFECTS}
    assert planted <= shown, sorted(planted - shown)


# ----------------------------------------------------------------------------- host refusals (no launch is reached)
EINVAL, EALIGN = -1, -2
A = 0x10000            # a 16-byte aligned address that is never dereferenced


def _refused(pkg, name, args, code, word):
    lib = pkg._lib.load()
    rc = getattr(lib, name)(*args)
    msg = lib.ssg_last_error()
    assert rc == code, (name, args, rc, msg)
    assert word in msg, (name, msg)


def _gemm(P=64, K=64, ldx=64, Kp=64, N=64, res=0, ldr=64, ldo=64, x=A, w=A, out=A):
    return (C.c_void_p(x), P, K, ldx, C.c_void_p(w), Kp, N, C.c_void_p(res), ldr, C.c_void_p(out), ldo, None)


@pytest.mark.parametrize('kw', [dict(K=60), dict(N=60), dict(ldx=68), dict(ldo=68), dict(res=A, ldr=68), dict(Kp=72), dict(Kp=32), dict(x=A + 8),
                                dict(out=A + 2), dict(res=A + 4)])
def test_gemm_refusals(pkg, kw):
    _refused(pkg, 'ssg_gemm_bf16', _gemm(**kw), EALIGN, b'gemm_bf16')


def test_gemm_null_and_wgrad_refusals(pkg):
    _refused(pkg, 'ssg_gemm_bf16', _gemm(P=0), EINVAL, b'gemm_bf16')
    _refused(pkg, 'ssg_gemm_bf16', _gemm(x=0), EINVAL, b'gemm_bf16')
    nbytes = pkg._lib.call('ssg_gemm_wgrad_bf16_workspace_bytes', 4133, 24, 264)

    def wg(M=24, N=264, ldd=32, ldx=272, dy=A, ws_bytes=nbytes):
        return (C.c_void_p(dy), ldd, C.c_void_p(A), ldx, 4133, M, N, C.c_void_p(A), C.c_void_p(A), ws_bytes, None)
    _refused(pkg, 'ssg_gemm_wgrad_bf16', wg(ws_bytes=nbytes - 1), EINVAL, b'gemm_wgrad_bf16: workspace')
    _refused(pkg, 'ssg_gemm_wgrad_bf16', wg(M=20), EALIGN, b'gemm_wgrad_bf16')
    _refused(pkg, 'ssg_gemm_wgrad_bf16', wg(ldd=36), EALIGN, b'gemm_wgrad_bf16')
    _refused(pkg, 'ssg_gemm_wgrad_bf16', wg(ldx=268), EALIGN, b'gemm_wgrad_bf16')
    _refused(pkg, 'ssg_gemm_wgrad_bf16', wg(dy=A + 8), EALIGN, b'gemm_wgrad_bf16')


@pytest.mark.parametrize('args', [(24, 40, 0, 64, 64), (24, 40, 0, 128, 32), (24, 40, 1, 128, 16), (24, 40, 1, 64, 32), (24, 40, 0, 128, 48), (0, 40, 0, 128, 64)])
def test_pack_refusals(pkg, args):
    O, I, tr, rows_pad, Kp = args
    _refused(pkg, 'ssg_pack_weights_bf16', (C.c_void_p(A), O, I, tr, rows_pad, Kp, C.c_void_p(A), None), EINVAL, b'pack_weights_bf16')


def _stem(Cin=3, Cout=32, ldx=4, KH=3, KW=3, stride=2, ldy=32):
    return dict(Cin=Cin, Cout=Cout, ldx=ldx, KH=KH, KW=KW, stride=stride, ldy=ldy)


@pytest.mark.parametrize('kw,code', [(dict(Cin=5), EINVAL), (dict(Cout=36, ldy=40), EINVAL), (dict(ldx=6), EINVAL), (dict(stride=3), EINVAL),
                                     (dict(KH=6, KW=6), EINVAL), (dict(ldy=24), EALIGN), (dict(ldy=36), EALIGN), (dict(KH=5, KW=5, Cout=168, ldy=168), EINVAL)])
def test_stem_refusals(pkg, kw, code):
    s = _stem(**kw)
    p = C.c_void_p(A)
    fwd = (p, 1, 16, 16, s['ldx'], p, s['Cout'], s['Cin'], s['KH'], s['KW'], s['stride'], 0, 0, 7, 7, p, s['ldy'], None)
    _refused(pkg, 'ssg_conv2d_thin_bf16', fwd, code, b'conv2d_thin_bf16')
    if 'ldy' not in kw or 'Cout' in kw and s['Cout'] != 168:
        wg = (p, 1, 16, 16, s['ldx'], p, s['ldy'], s['Cout'], s['Cin'], s['KH'], s['KW'], s['stride'], 0, 0, 7, 7, p, p, None)
        _refused(pkg, 'ssg_conv2d_thin_bf16_wgrad', wg, code, b'conv2d_thin_bf16_wgrad')
        dg = (p, s['ldy'], 1, 16, 16, p, s['Cout'], s['Cin'], s['KH'], s['KW'], s['stride'], 0, 0, 7, 7, p, s['ldx'], None)
        _refused(pkg, 'ssg_conv2d_thin_bf16_dgrad', dg, code, b'conv2d_thin_bf16_dgrad')


def test_stem_wgrad_group_limit_and_row_refusals(pkg):
    p = C.c_void_p(A)
    wg = lambda Cout, lddy, k: (p, 1, 16, 16, 4, p, lddy, Cout, 3, k, k, 2, 0, 0, 6, 6, p, p, None)
    _refused(pkg, 'ssg_conv2d_thin_bf16_wgrad', wg(88, 88, 5), EINVAL, b'conv2d_thin_bf16_wgrad: 36 pixels / 275')
    _refused(pkg, 'ssg_conv2d_thin_bf16_wgrad', wg(32, 24, 3), EALIGN, b'conv2d_thin_bf16_wgrad')
    _refused(pkg, 'ssg_conv2d_thin_bf16_wgrad', wg(32, 36, 3), EALIGN, b'conv2d_thin_bf16_wgrad: dy rows')


@pytest.mark.parametrize('name,word', [('ssg_convert_f32_to_bf16', b'convert_f32_to_bf16'), ('ssg_convert_bf16_to_f32', b'convert_bf16_to_f32')])
def test_convert_refusals(pkg, name, word):
    p = C.c_void_p(A)
    for ls, Cc, ld in ((8, 6, 8), (6, 4, 8), (8, 4, 6), (8, 0, 8)):
        _refused(pkg, name, (p, ls, 10, Cc, p, ld, None), EINVAL, word)


def test_add_refusals(pkg):
    p = C.c_void_p(A)
    for la, lb, Cc, lo in ((8, 8, 6, 8), (6, 8, 4, 8), (8, 6, 4, 8), (8, 8, 4, 6)):
        _refused(pkg, 'ssg_add_bf16', (p, la, p, lb, 10, Cc, p, lo, None), EINVAL, b'add_bf16')
    _refused(pkg, 'ssg_add_bf16', (p, 8, C.c_void_p(0), 8, 10, 4, p, 8, None), EINVAL, b'add_bf16')
