"""CPU: the host side of the fused clip + SGD step (optim.clip_sgd_step -> ssg_clamp_sgd_multi_f32): the entry is exported and
bound, it refuses a bad plan before any launch, _supported_sgd draws the line the trainers dispatch on, and the launch plan's
cache key carries the per-tensor first-step flags.  The arithmetic is tests/test_sgd_step_gpu.py's."""
import ctypes

import pytest
import torch

ENTRY = 'ssg_clamp_sgd_multi_f32'


def test_entry_is_exported_and_bound(pkg):
    assert ENTRY in pkg._lib.SIGNATURES
    assert hasattr(ctypes.CDLL(pkg._lib.LIB_PATH), ENTRY)
    fn = getattr(pkg._lib.load(), ENTRY)
    assert len(fn.argtypes) == 12 and fn.restype is ctypes.c_int


def test_bad_plan_returns_status_without_a_launch(pkg):
    """Validation is host code that runs before hipLaunchKernelGGL, so this needs no GPU."""
    lib = pkg._lib.load()
    one = ctypes.c_void_p(8)                         # never dereferenced: every call below fails validation
    hyper = (0.8, 1e-2, 0.9, 0.0, 1e-4, 1, None)
    for plan in ((None, None, None, None, 1), (None, one, one, one, 1), (one, one, one, None, 1),
                 (one, one, one, one, -1), (one, one, one, one, 0)):
        rc = getattr(lib, ENTRY)(*(plan + hyper))
        assert rc != 0 and ENTRY.encode() in lib.ssg_last_error(), (plan, rc, lib.ssg_last_error())
    # nesterov without momentum, or with dampening: what torch.optim.SGD's constructor refuses
    for mom, damp in ((0.0, 0.0), (0.9, 0.1)):
        rc = getattr(lib, ENTRY)(one, one, one, one, 1, 0.8, 1e-2, mom, damp, 0.0, 1, None)
        assert rc != 0 and ENTRY.encode() in lib.ssg_last_error()
    with pytest.raises(RuntimeError, match=ENTRY + ' failed'):
        pkg._lib.call(ENTRY, None, None, None, None, 0, 0.0, 1e-2, 0.0, 0.0, 0.0, 0, None)


def test_supported_sgd(pkg):
    ok = pkg.optim._supported_sgd

    def params():
        return [torch.zeros(3, requires_grad=True)]
    assert ok(torch.optim.SGD(params(), lr=0.1))
    assert ok(torch.optim.SGD(params(), lr=0.1, momentum=0.9, nesterov=True, weight_decay=1e-4))
    assert ok(torch.optim.SGD(params(), lr=0.1, momentum=0.9, dampening=0.1))
    assert ok(torch.optim.SGD([dict(params=params(), lr=0.1), dict(params=params(), lr=0.2, momentum=0.5)], lr=0.3))
    assert not ok(torch.optim.SGD(params(), lr=0.1, maximize=True))
    assert not ok(torch.optim.SGD(params(), lr=0.1, differentiable=True))
    assert not ok(torch.optim.SGD(params(), lr=torch.tensor(0.1)))
    assert not ok(torch.optim.SGD([dict(params=params()), dict(params=params(), maximize=True)], lr=0.1))   # one group is enough

    class MySGD(torch.optim.SGD):                    # a subclass may override step()
        pass
    assert not ok(MySGD(params(), lr=0.1))
    assert not ok(torch.optim.Adam(params(), lr=0.1))
    assert not pkg.optim._supported(torch.optim.SGD(params(), lr=0.1))                 # and Adam's predicate does not take an SGD
    with pytest.raises(NotImplementedError):
        pkg.optim.clip_sgd_step(torch.optim.SGD(params(), lr=0.1, maximize=True), 0.8)


def test_plan_key_carries_the_first_step_flags(pkg):
    """A tensor's second momentum step has the four addresses and the numel of its first and differs only in the flag: a
    plan found by addresses and sizes alone would overwrite the buffer with the gradient on every step."""
    optim = pkg.optim
    cpu = torch.device('cpu')
    ps = [torch.zeros(n, requires_grad=True) for n in (5000, 3)]
    for p in ps:
        p.grad = torch.zeros_like(p)
    bufs = [torch.zeros_like(p) for p in ps]
    optim._PLAN_CACHE.clear()
    plans = {}
    for first in ((True, True), (False, False), (True, False), (False, True)):
        plan = optim._sgd_plan(ps, bufs, first, cpu)
        assert all(plan is not other for other in plans.values()), first
        plans[first] = plan
        rec = plan[0].view(-1, 4)
        assert rec[:, 3].tolist() == [int(f) for f in first]
        assert rec[:, :3].tolist() == [[p.data_ptr(), p.grad.data_ptr(), b.data_ptr()] for p, b in zip(ps, bufs)]
        assert plan[1].tolist() == [5000, 3] and plan[2].tolist() == [0, 0, 1] and plan[3].tolist() == [0, 1, 0] and plan[4] == 3
    assert len(optim._PLAN_CACHE) == 4
    for first, plan in plans.items():
        assert optim._sgd_plan(ps, bufs, first, cpu) is plan                           # the same launch still hits
    # momentum == 0: no buffer, a null pointer in the record
    plan = optim._sgd_plan(ps, [None, None], (False, False), cpu)
    assert plan[0].view(-1, 4)[:, 2:].tolist() == [[0, 0], [0, 0]] and all(plan is not other for other in plans.values())
    # sizes stay part of the key (the comment on _cached_plan)
    small = ps[0].detach()[:4000].requires_grad_(True)
    small.grad = ps[0].grad[:4000]
    assert small.data_ptr() == ps[0].data_ptr()
    plan = optim._sgd_plan([small], [bufs[0][:4000]], (False,), cpu)
    assert plan[1].tolist() == [4000] and plan[4] == 1
