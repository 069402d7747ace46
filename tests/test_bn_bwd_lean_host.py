"""No GPU: the predicate of the 1-bit activation masks (ssg_bn_mask_ok), the host-side router that asks it, and the status the four
new launchers return for arguments they refuse.  Validation happens on the host before any launch, so the stand-in pointers
(16-byte aligned, never dereferenced) are safe here."""
import ctypes as C

import pytest
import torch

NONE, RELU, LRELU, SWISH = 0, 1, 2, 3
FAKE = C.c_void_p(0x1000)
NULL = C.c_void_p(0)


def test_predicate(pkg):
    ok = lambda c, act: pkg._lib.call('ssg_bn_mask_ok', c, act)
    for c in (8, 16, 64, 264, 4096):
        assert ok(c, RELU) == 1 and ok(c, LRELU) == 1
        assert ok(c, NONE) == 0 and ok(c, SWISH) == 0 and ok(c, 7) == 0
    for c in (0, -8, 1, 4, 12, 20, 65):
        assert ok(c, RELU) == 0 and ok(c, LRELU) == 0


def test_router_asks_the_switch_the_residual_the_dtype_and_the_predicate(pkg, monkeypatch):
    ops = pkg.ops
    x = ops.new_nhwc(1, 16, 3, 3, 'cpu', zero=True); r = ops.new_nhwc(1, 16, 3, 3, 'cpu', zero=True)
    x12 = ops.new_nhwc(1, 12, 3, 3, 'cpu', zero=True)
    assert ops.BN_BWD_LEAN_MIN > x.numel()
    for lean in (1, 2):
        monkeypatch.setattr(ops, 'BN_BWD_LEAN', lean)
        monkeypatch.setattr(ops, 'BN_BWD_LEAN_MIN', x.numel() if lean == 1 else 1 << 40)     # at the threshold under 1; 2 ignores it
        assert ops._bn_mask_route(x, r, RELU) is True and ops._bn_mask_route(x, r, LRELU) is True
        assert ops._bn_mask_route(x, None, RELU) is False          # no residual: the mask is recomputed from x
        assert ops._bn_mask_route(x, r, NONE) is False and ops._bn_mask_route(x, r, SWISH) is False
        assert ops._bn_mask_route(x12, x12, RELU) is False
        assert ops._bn_mask_route(x.to(torch.bfloat16), r, RELU) is False
    monkeypatch.setattr(ops, 'BN_BWD_LEAN', 0)
    assert ops._bn_mask_route(x, r, RELU) is False and ops._bn_lean() is False
    monkeypatch.setattr(ops, 'BN_BWD_LEAN', 1)
    monkeypatch.setattr(ops, 'BN_BWD_LEAN_MIN', x.numel() + 1)     # the size threshold holds under 1, not under 2
    assert ops._bn_mask_route(x, r, RELU) is False
    assert ops._bn_lean() is True                                  # the one-node conv -> BN -> act and the stem's sweep have no threshold
    monkeypatch.setattr(ops, 'BN_BWD_LEAN', 2)
    assert ops._bn_mask_route(x, r, RELU) is True


def _refused(pkg, name, *args):
    lib = pkg._lib.load()
    rc = getattr(lib, name)(*args)
    assert rc != 0, name
    assert name[len('ssg_'):-len('_f32')].encode() in lib.ssg_last_error(), lib.ssg_last_error()
    with pytest.raises(RuntimeError):
        pkg._lib.call(name, *args)


@pytest.mark.parametrize('c,act,mask,ldm', [(12, RELU, FAKE, 2), (16, NONE, FAKE, 2), (16, SWISH, FAKE, 2), (16, RELU, NULL, 2), (16, RELU, FAKE, 1)])
def test_mask_launchers_return_a_status(pkg, c, act, mask, ldm):
    P, ld = 10, 16
    _refused(pkg, 'ssg_bn_apply_mask_f32', FAKE, P, c, ld, FAKE, FAKE, FAKE, ld, act, 0.2, FAKE, ld, mask, ldm, None)
    _refused(pkg, 'ssg_bn_bwd_reduce_mask_f32', FAKE, mask, FAKE, P, c, ld, ldm, ld, FAKE, FAKE, act, 0.2, FAKE, 0, FAKE, None)
    _refused(pkg, 'ssg_bn_bwd_apply_mask_f32', FAKE, mask, FAKE, P, c, ld, ldm, ld, FAKE, FAKE, FAKE, FAKE, float(P), act, 0.2,
             FAKE, ld, FAKE, ld, FAKE, FAKE, None)
    if mask.value:                                               # (without a mask the sums form reads y or recomputes: not refused)
        _refused(pkg, 'ssg_bn_bwd_apply_sums_f32', FAKE, NULL, mask, FAKE, P, c, ld, 0, ldm, ld, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, float(P),
                 act, 0.2, FAKE, ld, NULL, 0, FAKE, FAKE, FAKE, FAKE, None)


def test_sums_launcher_returns_a_status(pkg):
    P, c, ld = 10, 16, 16

    def args(x=FAKE, y=NULL, mask=NULL, act=RELU, dx=FAKE, dxsum=FAKE, ws=FAKE, scale=FAKE, lddx=ld, cc=c):
        return (x, y, mask, FAKE, P, cc, ld, ld, 2, ld, FAKE, FAKE, FAKE, scale, scale, FAKE, float(P), act, 0.2, dx, lddx, NULL, 0,
                FAKE, FAKE, dxsum, ws, None)
    for bad in (args(x=NULL), args(dx=NULL), args(dxsum=NULL), args(ws=NULL), args(act=SWISH), args(y=FAKE, mask=FAKE),
                args(scale=NULL), args(lddx=8), args(cc=6), args(dx=C.c_void_p(0x1004))):
        _refused(pkg, 'ssg_bn_bwd_apply_sums_f32', *bad)
