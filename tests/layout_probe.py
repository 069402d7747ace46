"""Instrumentation for the NHWC memory contract (head of ops.py): an activation is [N, C, H, W] over an
[N, H, W, ld] buffer, ld a multiple of 4, ld >= C, pad lanes [C, pad4(C)) zero.  Plain helper module (not a conftest):

* GuardedAllocator -- drop-in for ops.new_nhwc.  Every allocation sits between two guard bands of whole 4-KiB pages, the
  whole buffer is filled with one canary bit pattern (a quiet NaN with a payload no kernel produces), and check() asserts
  afterwards that (a) both guards still hold the canary, (b) every real channel lane was written, (c) every pad lane is
  == 0 (a float compare: the canary, any other NaN and any value fail it; -0.0 is a zero).
* poisoned_slice / canary_slice -- a tensor that is a channel slice [c0, c0 + C) of a wider canary-filled buffer (pixel
  stride ld > C), for inputs and for destinations; check_slice() asserts guards and neighbouring lanes kept the canary.

Canaries are written with ordinary torch fills and compared as int32, never as floats (NaN != NaN, and a float compare would
not tell this NaN from another).  Everything works on CPU tensors too, which is how tests/test_layout_probe.py proves that
each violation is detected."""
import sys

import torch

CANARY_BITS = 0x7FC5A5A5            # quiet NaN, payload 0x45a5a5
PAGE_FLOATS = 1024                  # 4 KiB


def pad4(c):
    return (c + 3) // 4 * 4


def _bits(t):
    return t.view(torch.int32)


def canary_fill_(t):
    _bits(t).fill_(CANARY_BITS)
    return t


def is_canary(t):
    """Boolean mask: which fp32 elements of t still hold the canary bit pattern."""
    return _bits(t) == CANARY_BITS


def _sync(device):
    if torch.device(device).type == 'cuda':
        torch.cuda.synchronize()


def _first(mask2d, w, h):
    """(n, y, x, lane) of the first set element of a [pixels, lanes] mask."""
    idx = int(mask2d.reshape(-1).nonzero()[0])
    pix, lane = divmod(idx, mask2d.shape[1])
    n, rem = divmod(pix, h * w)
    y, x = divmod(rem, w)
    return n, y, x, lane


class _Alloc(object):
    __slots__ = ('buf', 'n', 'c', 'h', 'w', 'ld', 'zero', 'who', 'guard')

    def __init__(self, buf, n, c, h, w, ld, zero, who, guard):
        self.buf, self.n, self.c, self.h, self.w, self.ld, self.zero, self.who, self.guard = buf, n, c, h, w, ld, zero, who, guard

    def name(self):
        return 'new_nhwc(%d, %d, %d, %d, ld=%d%s) in %s()' % (self.n, self.c, self.h, self.w, self.ld, ', zero=True' if self.zero else '', self.who)

    def payload(self):
        g, size = self.guard, self.n * self.h * self.w * self.ld
        return self.buf[g:g + size].view(self.n * self.h * self.w, self.ld)

    def guards(self):
        g, size = self.guard, self.n * self.h * self.w * self.ld
        return self.buf[:g], self.buf[g + size:]


def _guarded(n, c, h, w, ld, device, guard, zero=False, c0=0):
    """(whole buffer, [n, c, h, w] base tensor over lanes [c0, c0 + c) of its [n, h, w, ld] payload)."""
    size = n * h * w * ld
    buf = torch.empty(guard + size + guard, device=device, dtype=torch.float32)
    canary_fill_(buf)
    if zero:
        buf[guard:guard + size].zero_()
    t = torch.empty(0, device=device, dtype=torch.float32).set_(
        buf.untyped_storage(), guard + c0, (n, c, h, w), (h * w * ld, 1, w * ld, ld))
    return buf, t


class GuardedAllocator(object):
    """alloc = GuardedAllocator(); alloc.install(monkeypatch, pkg); ...run ops...; alloc.check()."""

    def __init__(self, guard_pages=1):
        self.guard = guard_pages * PAGE_FLOATS
        self.records = []

    def __call__(self, n, c, h, w, device, ld=None, zero=False):
        ld = pad4(c) if ld is None else ld
        buf, t = _guarded(n, c, h, w, ld, device, self.guard, zero=zero)
        self.records.append(_Alloc(buf, n, c, h, w, ld, bool(zero), sys._getframe(1).f_code.co_name, self.guard))
        return t

    def install(self, monkeypatch, pkg):
        """Replace both names that hold ops.new_nhwc (bf16.py reaches it through `ops.`, blocks.py imported it by name);
        monkeypatch restores them on every exit path."""
        monkeypatch.setattr(pkg.ops, 'new_nhwc', self)
        monkeypatch.setattr(pkg.blocks, 'new_nhwc', self)
        return self

    def violations(self):
        """One message per violated property per allocation (all recorded allocations, after a device sync)."""
        if not self.records:
            return []
        _sync(self.records[0].buf.device)
        counts = []
        for a in self.records:
            front, back = a.guards()
            p = a.payload()
            c4 = pad4(a.c)
            unwritten = is_canary(p[:, :a.c]).sum() if not a.zero else torch.zeros((), dtype=torch.int64, device=p.device)
            padbad = (p[:, a.c:c4] != 0).sum() if c4 > a.c else torch.zeros((), dtype=torch.int64, device=p.device)
            counts.append(torch.stack([(~is_canary(front)).sum(), (~is_canary(back)).sum(), unwritten, padbad]))
        counts = torch.stack(counts).cpu().tolist()
        out = []
        for a, (nf, nb, nu, npad) in zip(self.records, counts):
            front, back = a.guards()
            p = a.payload()
            if nf:
                out.append('%s: front guard overwritten, %d floats, first %d floats before the tensor'
                           % (a.name(), nf, a.guard - int((~is_canary(front)).nonzero()[0])))
            if nb:
                out.append('%s: back guard overwritten, %d floats, first %d floats past the tensor'
                           % (a.name(), nb, int((~is_canary(back)).nonzero()[0])))
            if nu:
                out.append('%s: %d elements of real channel lanes never written, first (n, y, x, lane) = %s'
                           % (a.name(), nu, _first(is_canary(p[:, :a.c]), a.w, a.h)))
            if npad:
                n_, y_, x_, l_ = _first(p[:, a.c:pad4(a.c)] != 0, a.w, a.h)
                out.append('%s: %d pad-lane elements are not zero, first (n, y, x, lane) = %s'
                           % (a.name(), npad, (n_, y_, x_, a.c + l_)))
        return out

    def check(self):
        """Assert the three properties for every allocation recorded so far -- all of them again at every call, because a later
        kernel can overrun into an earlier tensor; the record must not be empty (a silently unpatched new_nhwc cannot pass)."""
        assert self.records, 'the guarded allocator saw no allocation: ops.new_nhwc was not the one in use'
        bad = self.violations()
        assert not bad, '%d layout violations:\n  %s' % (len(bad), '\n  '.join(bad))

    def frames(self):
        return sorted(set(a.who for a in self.records))


class _Slice(object):
    __slots__ = ('buf', 'n', 'c', 'h', 'w', 'ld', 'c0', 'guard')

    def name(self):
        return 'slice [%d, %d) of an [%d, %d, %d, ld=%d] buffer' % (self.c0, self.c0 + self.c, self.n, self.h, self.w, self.ld)


def canary_slice(n, c, h, w, ld, c0, dev, guard_pages=1):
    """[n, c, h, w] tensor over lanes [c0, c0 + c) of a guarded, canary-filled [n, h, w, ld] buffer (a destination)."""
    if c % 4 or c0 % 4 or ld % 4 or c0 + c > ld:
        raise ValueError('channel slice needs C %% 4 == 0, c0 %% 4 == 0, ld %% 4 == 0 and c0 + C <= ld (C=%d c0=%d ld=%d)' % (c, c0, ld))
    guard = guard_pages * PAGE_FLOATS
    buf, t = _guarded(n, c, h, w, ld, dev, guard, c0=c0)
    rec = _Slice()
    rec.buf, rec.n, rec.c, rec.h, rec.w, rec.ld, rec.c0, rec.guard = buf, n, c, h, w, ld, c0, guard
    t._layout_probe = rec
    return t


def poisoned_slice(x_cpu, ld, c0, dev):
    """The [N, C, H, W] view of x placed in lanes [c0, c0 + C) of a canary-filled, guarded [N, H, W, ld] device buffer."""
    n, c, h, w = x_cpu.shape
    t = canary_slice(n, c, h, w, ld, c0, dev)
    t.copy_(x_cpu.to(dtype=torch.float32))
    return t


def slice_violations(t, written=False):
    """Guards and neighbouring lanes of a canary_slice / poisoned_slice tensor must still hold the canary; with `written`
    (a destination) every element of the slice itself must have been written."""
    rec = t._layout_probe
    _sync(rec.buf.device)
    g, size = rec.guard, rec.n * rec.h * rec.w * rec.ld
    front, back = rec.buf[:g], rec.buf[g + size:]
    p = rec.buf[g:g + size].view(rec.n * rec.h * rec.w, rec.ld)
    out = []
    nf, nb = int((~is_canary(front)).sum()), int((~is_canary(back)).sum())
    if nf:
        out.append('%s: front guard overwritten, %d floats' % (rec.name(), nf))
    if nb:
        out.append('%s: back guard overwritten, %d floats' % (rec.name(), nb))
    neigh = ~is_canary(p)
    neigh[:, rec.c0:rec.c0 + rec.c] = False
    if int(neigh.sum()):
        out.append('%s: %d elements of neighbouring lanes overwritten, first (n, y, x, lane) = %s'
                   % (rec.name(), int(neigh.sum()), _first(neigh, rec.w, rec.h)))
    if written:
        own = is_canary(p[:, rec.c0:rec.c0 + rec.c])
        if int(own.sum()):
            n_, y_, x_, l_ = _first(own, rec.w, rec.h)
            out.append('%s: %d elements of the slice never written, first (n, y, x, lane) = %s'
                       % (rec.name(), int(own.sum()), (n_, y_, x_, rec.c0 + l_)))
    return out


def check_slice(t, written=False):
    bad = slice_violations(t, written)
    assert not bad, '%d layout violations:\n  %s' % (len(bad), '\n  '.join(bad))
