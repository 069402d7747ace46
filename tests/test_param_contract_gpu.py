"""The parameter contract: what dtype, device and strides a weight, bias, batch-norm affine, running statistic or
u / v vector may have at a public entry, and when a tensor derived from parameters (a packed weight, a BN fold, the SPADE
gamma|beta concat) is rebuilt.  Activations have tests/test_layout_contract_gpu.py; this is the same for the other operands.

A1  every entry of TABLE, every operand: the dense run, then the run with that operand as a view of equal values and other
    strides inside a storage that covers a dense read.  Outputs, input gradients, parameter gradients (by value) and in-place
    state must equal the dense run; an operand the kernels write in place (running statistics, u, v) may instead be refused with
    ValueError / TypeError / HipLibraryError before anything is launched.
A2  fp64 / fp16 / bf16 / CPU operands: a contract error naming the op and the operand before any library entry point is called
    (the `spy` fixture replaces `call` everywhere with a recorder that raises: nothing in A2 ever launches).
A3  whole models converted with .to(memory_format=torch.channels_last) against their unconverted twins.
B2  caches x events: after each event the next forward (and backward where the backward reads the cache) equals a fresh module
    built from cloned values that never held a cache.  The host half of B is tests/test_param_cache_host.py.  Two more caches
    have their cells elsewhere: the inference API's graph cache (tests/test_infer_gpu.py::test_graph_replay_follows_load_state_dict)
    and the optimizers' launch plans (tests/test_step_tail_gpu.py).

Match level: every dense run is made twice first.  Where the two agree bit for bit the strided / post-event run must agree bit for
bit too; where an op is not run-to-run reproducible the entry's `tol`, quoted from that op's existing test, is used instead and the
entry's name is printed ("tolerance branch")."""
import contextlib
import inspect
import math
import os
import re
import sys
import types
from collections import OrderedDict

import numpy as np
import pytest
import torch
import torch.nn as nn

from conftest import GOLDEN
from test_layout_contract_gpu import OP_TABLE
from test_ops_gpu import CONV_CASES, _close

pytestmark = pytest.mark.gpu

CANARY = 7.25
LAYOUT = dict(OP_TABLE)             # shapes and values of the smallest cases the ops already have
ALLOWED = (ValueError, TypeError)   # + HipLibraryError, added where the package is at hand (it subclasses RuntimeError)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _tup(y):
    return tuple(y) if isinstance(y, (tuple, list)) else (y,)


class _Launched(Exception):
    """Raised by the blocking spy in place of a library call."""


@pytest.fixture
def spy(pkg, monkeypatch):
    """Replaces `call` in _lib and in every package module that imported it.  rec.names records each entry point asked for;
    with rec.block the replacement raises instead of calling."""
    real = pkg._lib.call
    rec = types.SimpleNamespace(names=[], block=False)

    def fake(name, *args):
        rec.names.append(name)
        if rec.block:
            raise _Launched(name)
        return real(name, *args)
    hit = 0
    for mname, mod in list(sys.modules.items()):
        if mod is not None and (mname == pkg.__name__ or mname.startswith(pkg.__name__ + '.')) and mod.__dict__.get('call') is real:
            monkeypatch.setattr(mod, 'call', fake)
            hit += 1
    assert hit >= 4 and pkg.ops.call is fake and pkg.bf16.call is fake and pkg.blocks.call is fake and pkg._lib.call is fake
    return rec


def _contract_error(pkg, e):
    """ValueError / TypeError / HipLibraryError -- not a bare RuntimeError (what .view raises), not the spy's sentinel."""
    return isinstance(e, ALLOWED + (pkg._lib.HipLibraryError,))


# ----------------------------------------------------------------------------------------------------------- cases
class Case(object):
    """One prepared run: `xs` device inputs (leaves), `P` the operands by name (dense device tensors until set() replaces one),
    fn(xs, P) -> outputs.  diff: operands that receive a gradient; written: operands the kernels write in place."""

    def __init__(self, xs, P, fn, diff, written=(), fwd_only=False, no_grad=False, mod=None):
        self.xs, self.P, self.fn, self.diff, self.written = xs, P, fn, list(diff), list(written)
        self.fwd_only, self.no_grad, self.mod = fwd_only or no_grad, no_grad, mod
        if not self.fwd_only:
            for x in xs:
                if x.is_floating_point():
                    x.requires_grad_(True)
            if mod is None:
                for k in self.diff:
                    P[k].requires_grad_(True)

    def get(self, name):
        if self.mod is None:
            return self.P[name]
        m, leaf = _owner(self.mod, name)
        return m._parameters[leaf] if leaf in m._parameters else m._buffers[leaf]

    def set(self, name, t):
        if self.mod is None:
            self.P[name] = t.requires_grad_(True) if (name in self.diff and not self.fwd_only and t.is_floating_point()) else t
            return
        m, leaf = _owner(self.mod, name)
        if leaf in m._parameters:
            m._parameters[leaf] = nn.Parameter(t, requires_grad=t.is_floating_point())
        else:
            m._buffers[leaf] = t

    def run(self, seed=77):
        with (torch.no_grad() if self.no_grad else contextlib.nullcontext()):
            ys = _tup(self.fn(self.xs, self.P))
        res = OrderedDict(('y%d' % i, y.detach().clone()) for i, y in enumerate(ys))
        if not self.fwd_only:
            g = _gen(seed)
            dys = [torch.randn(y.shape, generator=g).to(y.dtype).to(y.device) for y in ys]
            torch.autograd.backward(list(ys), dys)
            for i, x in enumerate(self.xs):
                if x.is_floating_point():
                    res['dx%d' % i] = x.grad
            for k in self.diff:
                res['d:' + k] = self.get(k).grad
        for k in self.written:
            res['s:' + k] = self.get(k).detach().clone()
        torch.cuda.synchronize()
        return res


def _owner(mod, path):
    parts = path.split('.')
    for p in parts[:-1]:
        mod = getattr(mod, p)
    return mod, parts[-1]


def _module_case(mod, xs, fwd=None, no_grad=False):
    P = OrderedDict(list(mod.named_parameters()) + [(k, b) for k, b in mod.named_buffers() if b.is_floating_point()])
    diff = [k for k, _ in mod.named_parameters()]
    written = [k for k, b in mod.named_buffers() if b.is_floating_point()]
    return Case(xs, P, (lambda xs_, P_: (fwd or mod)(*xs_)), diff, written, no_grad=no_grad, mod=mod)


def _nhwc(pkg, dev, x):
    return pkg.ops.to_nhwc(x.to(dev))


def _bn_holder(P, training, track=True):
    return types.SimpleNamespace(training=training, track_running_stats=track, momentum=0.1, eps=1e-5, weight=P['weight'], bias=P['bias'],
                                 running_mean=P.get('running_mean'), running_var=P.get('running_var'), num_batches_tracked=None)


class Entry(object):
    """name; covers: the public names this entry exercises; op: the name contract errors carry (None for modules: any known op);
    make(pkg, dev) -> Case; names: operand -> the name the error carries (default: the operand's own, modules: its last part);
    tol: (rtol, atol) of the tolerance branch."""

    def __init__(self, name, covers, op, make, tol, names=None, composite=False):
        self.name, self.covers, self.op, self.make, self.tol, self.names = name, set(covers), op, make, tol, names or {}
        # composite: a module that calls several public entries in turn (MBConvBlock).  An entry refuses its own operand before IT
        # launches, but the entries before it have run: such a module is in A1 only -- in A2 the blocking spy would stop it at its
        # first entry, and letting it run up to the bad operand is exactly the launch A2 must not make.  Each entry it calls has
        # its own row.
        self.composite = composite


def _conv_entry(name, shape, precision='fp32', x2=False, res=False, bias=True, covers=('conv2d',)):
    n, cin, cout, h, w, k, s, p = shape
    c1 = cin // 2 if x2 else cin

    def make(pkg, dev):
        g = _gen(cin * 7 + cout)
        xs = [torch.randn(n, c1, h, w, generator=g)] + ([torch.randn(n, cin - c1, h, w, generator=g)] if x2 else [])
        oh, ow = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
        if res:
            xs.append(torch.randn(n, cout, oh, ow, generator=g))
        P = OrderedDict(weight=(torch.randn(cout, cin, k, k, generator=g) / math.sqrt(cin * k * k)).to(dev))
        if bias:
            P['bias'] = torch.randn(cout, generator=g).to(dev)

        def fn(xs_, P_):
            return pkg.ops.conv2d(xs_[0], P_['weight'], P_.get('bias'), s, p, act=pkg._lib.ACT_LRELU, slope=0.2, x2=xs_[1] if x2 else None,
                                  res=xs_[-1] if res else None, precision=precision)
        return Case([_nhwc(pkg, dev, x) for x in xs], P, fn, list(P))
    # test_conv2d_fwd_bwd (tests/test_ops_gpu.py): the weight gradient's (2e-5, 2e-6 * sqrt(n * h * w)), the widest of its four bounds
    return Entry(name, covers, 'conv2d', make, (2e-5, max(1e-5, 2e-6 * math.sqrt(n * h * w))))


X1_SHAPE = (1, 64, 64, 9, 17, 3, 1, 1)         # the bf16x1 / bf16x2 predicates: C1, C2 % 32 == 0, Cout % 64 == 0, W >= 17


def _conv_x1_infer_entry():
    n, cin, cout, h, w = X1_SHAPE[:5]

    def make(pkg, dev):
        g = _gen(41)
        xs = [torch.randn(n, cin // 2, h, w, generator=g), torch.randn(n, cin // 2, h, w, generator=g), torch.randn(n, cout, h, w, generator=g)]
        P = OrderedDict(weight=(torch.randn(cout, cin, 3, 3, generator=g) / 24).to(dev), bias=torch.randn(cout, generator=g).to(dev))
        return Case([_nhwc(pkg, dev, x) for x in xs], P,
                    lambda xs_, P_: pkg.ops.conv2d_bf16x1(xs_[0], P_['weight'], P_['bias'], act=pkg._lib.ACT_RELU, x2=xs_[1], res=xs_[2]), [], no_grad=True)
    # test_conv_bf16x1_gpu.py bounds the kernel by (2^-8 + 2^-18) * conv(|x|, |w|); two runs of it differ by far less than the fp32 bound
    return Entry('conv2d_bf16x1', ('conv2d_bf16x1',), 'conv2d_bf16x1', make, (2e-5, 1e-5))


def _conv_sn_entry():
    def make(pkg, dev):
        c = LAYOUT['conv2d_sn']()
        g = _gen(13)
        P = OrderedDict(weight_orig=c['ps'][0].to(dev), bias=c['ps'][1].to(dev),
                        u=torch.nn.functional.normalize(torch.randn(32, generator=g), dim=0).to(dev),
                        v=torch.nn.functional.normalize(torch.randn(144, generator=g), dim=0).to(dev))
        return Case([_nhwc(pkg, dev, c['xs'][0])], P,
                    lambda xs_, P_: pkg.ops.conv2d_sn(xs_[0], P_['weight_orig'], P_['u'], P_['v'], P_['bias'], 1, 1, act=pkg._lib.ACT_LRELU, slope=0.2),
                    ['weight_orig', 'bias'], written=['u', 'v'])
    # tests/test_layout_contract_gpu.py::_conv_sn_case: conv2d's formulas, the weight gradient's (2e-5, 2e-6 * sqrt(2 * 256))
    return Entry('conv2d_sn', ('conv2d_sn',), 'conv2d_sn', make, (2e-5, 2e-6 * math.sqrt(512)))


def _sn_weight_entry():
    def make(pkg, dev):
        c = LAYOUT['conv2d_sn']()
        g = _gen(14)
        P = OrderedDict(weight_orig=c['ps'][0].to(dev), u=torch.nn.functional.normalize(torch.randn(32, generator=g), dim=0).to(dev),
                        v=torch.nn.functional.normalize(torch.randn(144, generator=g), dim=0).to(dev))
        return Case([], P, lambda xs_, P_: pkg.ops.spectral_norm_weight(P_['weight_orig'], P_['u'], P_['v'])[0], ['weight_orig'], written=['u', 'v'])
    return Entry('spectral_norm_weight', ('spectral_norm_weight',), 'spectral_norm_weight', make, (2e-5, 1e-5))   # test_unwired_gpu.py: 2e-5 of the weight


def _dwconv_entry():
    key = 'dwconv2d-1-16-12-14-3-2-1'

    def make(pkg, dev):
        c = LAYOUT[key]()
        P = OrderedDict(weight=c['ps'][0].to(dev), bias=c['ps'][1].to(dev))
        return Case([_nhwc(pkg, dev, c['xs'][0])], P, lambda xs_, P_: pkg.ops.dwconv2d(xs_[0], P_['weight'], P_['bias'], 2, 1), list(P))
    return Entry('dwconv2d', ('dwconv2d',), 'dwconv2d', make, (2e-5, 2e-5 * math.sqrt(12 * 14)))       # test_dwconv2d: the weight gradient's bound


def _linear_entry(n, k, o):
    def make(pkg, dev):
        g = _gen(n * 100 + k)
        x = torch.randn(n, k, generator=g).to(dev)
        P = OrderedDict(weight=(torch.randn(o, k, generator=g) / math.sqrt(k)).to(dev), bias=torch.randn(o, generator=g).to(dev))
        return Case([x], P, lambda xs_, P_: pkg.ops.linear(xs_[0], P_['weight'], P_['bias'], act=pkg._lib.ACT_LRELU, slope=0.2), list(P))
    return Entry('linear-%dx%dx%d' % (n, k, o), ('linear',), 'linear', make, (2e-5, 2e-5))               # test_linear


def _bn_entry(mode):
    """mode: train | train-nostats | eval (no_grad) | frozen (eval with autograd)."""
    key = 'batch_norm_act-train-c8'                # [2, 8, 8, 9], relu, no residual

    def make(pkg, dev):
        c = LAYOUT[key]()
        g = _gen(6)
        P = OrderedDict(weight=c['ps'][0].to(dev), bias=c['ps'][1].to(dev))
        if mode != 'train-nostats':
            P['running_mean'] = torch.randn(8, generator=g).to(dev); P['running_var'] = (torch.rand(8, generator=g) + 0.5).to(dev)

        def fn(xs_, P_):
            bn = _bn_holder(P_, mode.startswith('train'), track=mode != 'train-nostats')
            return pkg.ops.batch_norm_act(xs_[0], bn, act=pkg._lib.ACT_RELU)
        stats = ['running_mean', 'running_var'] if mode != 'train-nostats' else []
        return Case([_nhwc(pkg, dev, c['xs'][0])], P, fn, ['weight', 'bias'], written=stats, no_grad=mode == 'eval')
    names = {k: 'bn.' + k for k in ('weight', 'bias', 'running_mean', 'running_var')}
    return Entry('batch_norm_act-' + mode, ('batch_norm_act',), 'batch_norm_act', make, (1e-4, 1e-4), names)     # test_batch_norm_act: dweight / dbias


def _se_entry():
    def make(pkg, dev):
        n, c, s = 4, 144, 6                         # test_se_gate_matches_the_two_convs' first shape
        torch.manual_seed(5 + c)
        red = nn.Conv2d(c, s, 1); exp = nn.Conv2d(s, c, 1)
        P = OrderedDict([('reduce_conv.weight', red.weight.detach().to(dev)), ('reduce_conv.bias', red.bias.detach().to(dev)),
                         ('expand_conv.weight', exp.weight.detach().to(dev)), ('expand_conv.bias', exp.bias.detach().to(dev))])

        def fn(xs_, P_):
            r = types.SimpleNamespace(weight=P_['reduce_conv.weight'], bias=P_['reduce_conv.bias'])
            e = types.SimpleNamespace(weight=P_['expand_conv.weight'], bias=P_['expand_conv.bias'])
            out = pkg.ops.se_gate(xs_[0], r, e)
            assert out is not None
            return out
        return Case([_nhwc(pkg, dev, torch.randn(n, c, 1, 1, generator=_gen(9)) * 0.7)], P, fn, list(P))
    return Entry('se_gate', ('se_gate',), 'se_gate', make, (1e-5, 2e-6))                 # tests/test_round3_gpu.py: 2e-6 * max(ref, 1) + 1e-5 * ref


def _bf16_entries():
    def thin(pkg, dev):
        g = _gen(3)                                 # test_stem_conv_bf16's k3 stride-2 form on a smaller image
        P = OrderedDict(weight=(torch.randn(8, 3, 3, 3, generator=g) / 5).to(dev))
        return Case([_nhwc(pkg, dev, torch.randn(1, 3, 20, 25, generator=g))], P, lambda xs_, P_: pkg.bf16.conv_thin(xs_[0], P_['weight'], 2, (0, 1, 0, 1)), ['weight'])

    def x_bf16(pkg, dev, shape, seed):
        return pkg.bf16.to_bf16(_nhwc(pkg, dev, torch.randn(*shape, generator=_gen(seed)))).detach()

    def c1x1(pkg, dev):                             # P = 130 pixels, K = 8, N = 8: one ragged row tile
        P = OrderedDict(weight=(torch.randn(8, 8, 1, 1, generator=_gen(4)) / 3).to(dev))
        return Case([x_bf16(pkg, dev, (1, 8, 10, 13), 5)], P, lambda xs_, P_: pkg.bf16.conv1x1(xs_[0], P_['weight']), ['weight'])

    def bn(pkg, dev):
        g = _gen(6)
        P = OrderedDict(weight=(torch.rand(8, generator=g) + 0.5).to(dev), bias=torch.randn(8, generator=g).to(dev),
                        running_mean=torch.randn(8, generator=g).to(dev), running_var=(torch.rand(8, generator=g) + 0.5).to(dev))
        return Case([x_bf16(pkg, dev, (2, 8, 6, 7), 7)], P,
                    lambda xs_, P_: pkg.bf16.batch_norm_act(xs_[0], _bn_holder(P_, True), act=pkg.bf16.ACT_SWISH), ['weight', 'bias'],
                    written=['running_mean', 'running_var'])

    def bn_eval(pkg, dev):
        c = bn(pkg, dev)
        return Case(c.xs, c.P, lambda xs_, P_: pkg.bf16.batch_norm_act(xs_[0], _bn_holder(P_, False)), [], written=['running_mean', 'running_var'], no_grad=True)

    def dw(pkg, dev):
        P = OrderedDict(weight=(torch.randn(8, 1, 3, 3, generator=_gen(8)) / 3).to(dev))
        return Case([x_bf16(pkg, dev, (1, 8, 9, 10), 9)], P, lambda xs_, P_: pkg.bf16.dwconv2d(xs_[0], P_['weight'], 1, 1), ['weight'])
    bnn = {k: 'bn.' + k for k in ('weight', 'bias', 'running_mean', 'running_var')}
    # tests/test_bf16_gpu.py bounds these kernels by a few bf16 roundings of the tensor's max (2.5e-2 forward, 4e-2 gradients)
    return [Entry('bf16.conv_thin', ('bf16.conv_thin',), 'bf16.conv_thin', thin, (4e-2, 0)),
            Entry('bf16.conv1x1', ('bf16.conv1x1',), 'bf16.conv1x1', c1x1, (4e-2, 0)),
            Entry('bf16.batch_norm_act-train', ('bf16.batch_norm_act',), 'bf16.batch_norm_act', bn, (4e-2, 0), bnn),
            Entry('bf16.batch_norm_act-eval', ('bf16.batch_norm_act',), 'bf16.batch_norm_act', bn_eval, (4e-2, 0), bnn),
            Entry('bf16.dwconv2d', ('bf16.dwconv2d',), 'bf16.dwconv2d', dw, (4e-2, 0))]


def _randomize_bn(mod, seed=2):
    g = _gen(seed)
    with torch.no_grad():
        for m in mod.modules():
            if isinstance(m, nn.modules.batchnorm._BatchNorm) and m.affine:
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5); m.bias.copy_(torch.randn(m.bias.shape, generator=g))
                m.running_mean.copy_(torch.randn(m.bias.shape, generator=g) * 0.3); m.running_var.copy_(torch.rand(m.bias.shape, generator=g) + 0.5)
    return mod


def _make_block(pkg, dev, route='train'):
    torch.manual_seed(11)
    m = _randomize_bn(pkg.archs.BasicBlock(16, 24)).to(dev)     # tests/test_layout_contract_gpu.py's smallest block: a 1x1 shortcut
    m.train(route in ('train', 'mixed'))
    if route == 'mixed':
        m.bn1.eval()
    return m


def _block_entry(route):
    def make(pkg, dev):
        m = _make_block(pkg, dev, route)
        with (torch.no_grad() if route == 'cached_eval' else contextlib.nullcontext()):
            assert m._route() == route
        return _module_case(m, [_nhwc(pkg, dev, torch.randn(2, 16, 12, 13, generator=_gen(12)))], no_grad=route == 'cached_eval')
    return Entry('BasicBlock-' + route, ('BasicBlock',), None, make, (1e-4, 2e-5))          # tests/test_blocks_gpu.py::_check


def _make_spade(pkg, dev):
    torch.manual_seed(12)
    return pkg.normalization.SPADE('spadebatch3x3', 64, 3, 4).to(dev).train()


def _spade_x(pkg, dev):
    return _nhwc(pkg, dev, torch.randn(1, 64, 19, 17, generator=_gen(15)))


def _spade_entry():
    def make(pkg, dev):
        m = _make_spade(pkg, dev)
        c = _module_case(m, [_spade_x(pkg, dev)], fwd=lambda x: m(x, x))
        c.written = []                              # param_free_norm's buffers are part of the state_dict and never read
        for k in [k for k in c.P if k.startswith('param_free_norm')]:
            del c.P[k]
        return c
    return Entry('SPADE', ('SPADE',), None, make, (2e-4, 1e-6))                              # test_spade_fused_gamma_beta_modulate's parameter bound


def _make_mbconv(pkg, dev, tag='mb_b'):
    gold = np.load(os.path.join(GOLDEN, 'unwired.npz'))
    E = pkg.efficientnet_pytorch
    k, s, inp, out, e, hw = [int(v) for v in gold[tag + '_cfg']]
    gp = E.GlobalParams(batch_norm_momentum=0.99, batch_norm_epsilon=1e-3, dropout_rate=0.2, num_classes=10, width_coefficient=1.0,
                        depth_coefficient=1.0, depth_divisor=8, min_depth=None, drop_connect_rate=0.2, image_size=224)
    ba = E.BlockArgs(kernel_size=k, num_repeat=1, input_filters=inp, output_filters=out, expand_ratio=e, id_skip=True, stride=[s], se_ratio=0.25)
    torch.manual_seed(35)
    return E.MBConvBlock(ba, gp).to(dev).train(), torch.from_numpy(gold[tag + '_x'])


def _mbconv_entry(family):
    def make(pkg, dev):
        m, x = _make_mbconv(pkg, dev)
        x = _nhwc(pkg, dev, x)
        if family == 'bf16':
            return _module_case(m, [pkg.bf16.to_bf16(x).detach()])
        return _module_case(m, [x])
    # test_mbconv_block_bf16: 4e-2 of the tensor's max; tests/test_unwired_gpu.py bounds the fp32 block's gradients by 1e-4
    return Entry('MBConvBlock-' + family, ('MBConvBlock',), None, make, (4e-2, 0) if family == 'bf16' else (1e-4, 2e-5), composite=True)


def _table():
    c0 = CONV_CASES[0][:8]                          # (2, 16, 32, 20, 24, 3, 1, 1): the first conv case of tests/test_ops_gpu.py
    t = [_conv_entry('conv2d-fp32', c0), _conv_entry('conv2d-fp32-nobias', c0, bias=False), _conv_entry('conv2d-fp32-x2-res', c0, x2=True, res=True),
         _conv_entry('conv2d-fp32-s2', CONV_CASES[9][:8]),
         _conv_entry('conv2d-bf16x1-x2-res', X1_SHAPE, 'bf16x1', x2=True, res=True), _conv_entry('conv2d-bf16x2-x2-res', X1_SHAPE, 'bf16x2', x2=True, res=True),
         _conv_entry('conv2d-bf16x1', X1_SHAPE, 'bf16x1'), _conv_entry('conv2d-bf16x2-nobias', X1_SHAPE, 'bf16x2', bias=False),
         _conv_x1_infer_entry(), _conv_sn_entry(), _sn_weight_entry(), _dwconv_entry(), _linear_entry(2, 64, 32), _linear_entry(3, 6, 5)]
    t += [_bn_entry(m) for m in ('train', 'train-nostats', 'eval', 'frozen')]
    t += [_se_entry()] + _bf16_entries()
    t += [_block_entry(r) for r in ('train', 'cached_eval', 'frozen', 'mixed')]
    t += [_spade_entry(), _mbconv_entry('fp32'), _mbconv_entry('bf16')]
    return t


TABLE = _table()
ENTRY = {e.name: e for e in TABLE}
# names an operand of a public entry goes by in its signature: a parameter, a module that holds some, or a vector the kernels update
PARAM_ARGS = {'weight', 'bias', 'bn', 'weight_orig', 'u', 'v', 'reduce_conv', 'expand_conv'}
# public names of ops.__all__ / bf16 without such an operand: activations (tests/test_layout_contract_gpu.py) or no tensor at all
NO_PARAM_OPERAND = {
    'ops': ['max_pool2x2', 'max_pool2x2_skip', 'max_unpool2x2', 'upsample2x_bilinear', 'upsample2x_nearest', 'spade_modulate', 'adaptive_avgpool_flat',
            'seg_loss', 'bce_with_logits_const', 'nan_to_zero_', 'to_nhwc', 'new_nhwc', 'bump_weight_epoch', 'swish', 'sigmoid', 'gaussian', 'mul',
            'global_avgpool', 'channel_scale'],
    'bf16': ['new_bf16', 'as_bf16', 'to_bf16', 'to_f32', 'global_avgpool', 'channel_scale', 'add'],
}


def test_table_covers_every_entry_with_a_parameter_operand(pkg):
    covered = set().union(*[e.covers for e in TABLE])
    for mod, names, prefix in ((pkg.ops, list(pkg.ops.__all__) + ['se_gate', 'conv2d_bf16x1'], ''),
                               (pkg.bf16, [n for n, f in vars(pkg.bf16).items() if inspect.isfunction(f) and not n.startswith('_')
                                           and f.__module__ == pkg.bf16.__name__], 'bf16.')):
        exempt = NO_PARAM_OPERAND['bf16' if prefix else 'ops']
        for n in names:
            takes = bool(PARAM_ARGS & set(inspect.signature(getattr(mod, n)).parameters))
            if takes:
                assert prefix + n in covered, '%s%s takes a parameter operand and has no entry in TABLE' % (prefix, n)
                assert n not in exempt, n
            else:
                assert n in exempt, '%s%s: neither in TABLE nor listed in NO_PARAM_OPERAND' % (prefix, n)
        assert set(exempt) <= set(names), sorted(set(exempt) - set(names))
    assert {'BasicBlock', 'SPADE', 'MBConvBlock'} <= covered
    assert {'BasicBlock-' + r for r in ('train', 'cached_eval', 'frozen', 'mixed')} <= set(ENTRY)


# ----------------------------------------------------------------------------------------------------------- dense baselines
_DENSE = {}


def _dense(pkg, dev, entry):
    """(result of the dense run, exact): two dense runs, each on a freshly made case; exact = they agree bit for bit."""
    if entry.name not in _DENSE:
        r0 = entry.make(pkg, dev).run()
        r1 = entry.make(pkg, dev).run()
        assert list(r0) == list(r1)
        exact = all((r0[k] is None and r1[k] is None) or torch.equal(r0[k], r1[k]) for k in r0)
        if not exact:
            print('tolerance branch: %s is not run-to-run reproducible' % entry.name)
        _DENSE[entry.name] = (r0, exact)
    return _DENSE[entry.name]


def _same(got, ref, exact, tol, what):
    assert list(got) == list(ref), what
    for k in ref:
        a, b = got[k], ref[k]
        assert (a is None) == (b is None), '%s: %s' % (what, k)
        if b is None:
            continue
        assert tuple(a.shape) == tuple(b.shape) and a.dtype == b.dtype, '%s: %s' % (what, k)
        if exact:
            assert torch.equal(a, b), '%s: %s differs from the dense run (max |diff| %.3e of max %.3e)' % (
                what, k, (a.double() - b.double()).abs().max().item(), b.double().abs().max().item())
        else:
            _close(a, b, tol[0], tol[1], '%s: %s' % (what, k))


def _variants(t):
    """(label, view of equal values and other strides, the canary-filled elements between / behind the view's or None).  Every
    view lives in a storage that extends at least numel() elements past its data_ptr(): a dense misread stays inside it."""
    if t.dim() == 1:
        buf = torch.full((2 * t.numel(),), CANARY, device=t.device, dtype=t.dtype)
        buf[::2].copy_(t)
        yield 'every-other', buf[::2], buf[1::2]
    elif t.dim() == 2:
        o, k = t.shape
        big = torch.full((o, k + 4), CANARY, device=t.device, dtype=t.dtype)
        big[:, :k].copy_(t)
        yield 'row-strided', big[:, :k], big[:, k:]
        yield 'column-major', t.t().contiguous().t(), None
    else:
        v = t.contiguous(memory_format=torch.channels_last)
        if not v.is_contiguous():
            yield 'channels_last', v, None
        else:                                       # I = 1 or a 1x1 kernel: channels_last is the dense layout; a channel slice is not
            o, i, kh, kw = t.shape
            big = torch.full((o, i + 1, kh, kw), CANARY, device=t.device, dtype=t.dtype)
            big[:, :i].copy_(t)
            yield 'channel-slice', big[:, :i], big[:, i:]


@pytest.mark.parametrize('name', [e.name for e in TABLE])
def test_a1_strided_operands(pkg, dev, spy, name):
    entry = ENTRY[name]
    ref, exact = _dense(pkg, dev, entry)
    probe = entry.make(pkg, dev)
    operands = list(probe.P)
    assert operands, name
    ran = 0
    for op_name in operands:
        labels = [v[0] for v in _variants(probe.get(op_name).detach())]
        for label in labels:
            case = entry.make(pkg, dev)
            dense_t = case.get(op_name).detach().clone()
            view, gap = [(v, g) for l, v, g in _variants(dense_t) if l == label][0]
            assert not view.is_contiguous() and torch.equal(view, dense_t), (name, op_name, label)
            assert view.untyped_storage().nbytes() - (view.data_ptr() - view.untyped_storage().data_ptr()) >= view.numel() * view.element_size()
            case.set(op_name, view)
            what = '%s, %s as %s' % (name, op_name, label)
            spy.names.clear()
            try:
                got = case.run()
            except Exception as e:                  # noqa: BLE001 -- classified right below
                assert _contract_error(pkg, e), '%s: %s: %s' % (what, type(e).__name__, e)
                assert op_name in case.written, '%s: refused, but the kernels only read this operand: %s' % (what, e)
                assert entry.composite or spy.names == [], '%s: refused after %s' % (what, spy.names[:3])
                ran += 1
                continue
            _same(got, ref, exact, entry.tol, what)
            if op_name in case.written:              # in-place state read back through the view, and nothing written beside it
                assert torch.equal(case.get(op_name).detach(), got['s:' + op_name])
            if gap is not None:
                assert bool((gap == CANARY).all()), '%s: the elements between the view\'s were written' % what
            ran += 1
    assert ran >= len(operands)


# ----------------------------------------------------------------------------------------------------------- A2
KNOWN_OPS = ('conv2d', 'conv2d_bf16x1', 'conv2d_sn', 'dwconv2d', 'linear', 'batch_norm_act', 'se_gate', 'spectral_norm_weight', 'bf16.conv_thin',
             'bf16.conv1x1', 'bf16.batch_norm_act', 'bf16.dwconv2d', 'basic_block', 'frozen_basic_block', 'spade_self', 'BasicBlock')


def _bad(t, kind):
    if kind == 'cpu':
        return t.detach().cpu().clone()
    return t.detach().to({'fp64': torch.float64, 'fp16': torch.float16, 'bf16': torch.bfloat16}[kind])


@pytest.mark.parametrize('kind', ['fp64', 'fp16', 'bf16', 'cpu'])
@pytest.mark.parametrize('name', [e.name for e in TABLE if not e.composite])
def test_a2_dtype_and_device(pkg, dev, spy, name, kind):
    """Parameters are fp32 in both tensor families (bf16.py keeps parameters, statistics and gates in fp32), so fp64 / fp16 / bf16
    are the wrong dtypes at every entry.  The spy blocks: the bad operand never reaches a kernel."""
    entry = ENTRY[name]
    operands = list(entry.make(pkg, dev).P)
    for op_name in operands:
        case = entry.make(pkg, dev)                 # (placing the inputs may convert layouts: before the spy blocks)
        case.set(op_name, _bad(case.get(op_name), kind))
        torch.cuda.synchronize()
        spy.names.clear(); spy.block = True
        try:
            with pytest.raises(Exception) as ei:
                case.run()
        finally:
            spy.block = False
        what = '%s, %s as %s' % (name, op_name, kind)
        e = ei.value
        assert spy.names == [], '%s: a library entry point was asked for first: %s' % (what, spy.names[:3])
        assert _contract_error(pkg, e), '%s: %s: %s' % (what, type(e).__name__, e)
        msg = str(e)
        said = entry.names.get(op_name, op_name if entry.op else op_name.split('.')[-1])
        assert said in msg, '%s: the error does not name the operand %r: %s' % (what, said, msg)
        if entry.op:
            assert msg.startswith(entry.op + ':'), '%s: the error does not name the op %r: %s' % (what, entry.op, msg)
        else:
            assert any(msg.startswith(o + ':') for o in KNOWN_OPS), '%s: the error names no op: %s' % (what, msg)


# ----------------------------------------------------------------------------------------------------------- A3
def _model_makers(pkg, dev):
    def gen():
        torch.manual_seed(41)
        m = pkg.models_seg_gan.Generator(dict(arch='UNet_R_SS_v2', num_classes=3, input_channels=3, deep_supervision=False))
        return _randomize_bn(m).to(dev), torch.randn(2, 3, 64, 64, generator=_gen(1))

    def disc():
        torch.manual_seed(14)
        gold = np.load(os.path.join(GOLDEN, 'blocks.npz'))
        return pkg.models_seg_gan.Discriminator(3, 3, 8, 8, 1024).to(dev), torch.from_numpy(gold['d_64_x'])

    def block():
        return _make_block(pkg, dev), torch.randn(2, 16, 12, 13, generator=_gen(12))

    def spade():
        return _make_spade(pkg, dev), torch.randn(1, 64, 19, 17, generator=_gen(15))
    return dict(generator=gen, discriminator=disc, BasicBlock=block, SPADE=spade)


def _model_run(m, x, dev, train):
    m.train(train)
    m.zero_grad(set_to_none=True)
    xd = x.to(dev)
    res = OrderedDict()
    if train:
        ys = _tup(m(xd))
        g = _gen(5)
        torch.autograd.backward(list(ys), [torch.randn(y.shape, generator=g).to(dev) for y in ys])
        for k, p in m.named_parameters():
            res['d:' + k] = p.grad
    else:
        with torch.no_grad():
            ys = _tup(m(xd))
    for i, y in enumerate(ys):
        res['y%d' % i] = y.detach().clone()
    torch.cuda.synchronize()
    return res


@pytest.mark.parametrize('which', ['generator', 'discriminator', 'BasicBlock', 'SPADE'])
def test_a3_channels_last_model_matches_its_twin(pkg, dev, which):
    make = _model_makers(pkg, dev)[which]
    # tests/test_blocks_gpu.py::_check (2e-5 forward, 1e-4 of the gradient's max) for the tolerance branch
    tol = (1e-4, 2e-5)
    for train in (False, True):                     # eval first: it reads the running statistics the train forward then moves
        a, x = make(); b, _ = make(); c, _ = make()
        c = c.to(memory_format=torch.channels_last)
        strided = [k for k, p in c.named_parameters() if not p.is_contiguous()]
        assert strided, '%s: the conversion restrided no parameter' % which
        ra, rb = _model_run(a, x, dev, train), _model_run(b, x, dev, train)
        exact = all((ra[k] is None and rb[k] is None) or torch.equal(ra[k], rb[k]) for k in ra)
        if not exact:
            print('tolerance branch: model %s (%s) is not run-to-run reproducible' % (which, 'train' if train else 'eval'))
        rc = _model_run(c, x, dev, train)
        _same(rc, ra, exact, tol, '%s %s, channels_last' % (which, 'train' if train else 'eval'))
        if not train:                               # once more: now through the filled fold / pack caches
            _same(_model_run(c, x, dev, train), ra, exact, tol, '%s eval, channels_last, cached' % which)


# ----------------------------------------------------------------------------------------------------------- B2: caches x events
class _ConvMod(nn.Module):
    def __init__(self, pkg, cin, cout, precision='fp32', bias=True, weight=None):
        super().__init__()
        self.pkg, self.precision = pkg, precision
        self.weight = weight if weight is not None else nn.Parameter(torch.randn(cout, cin, 3, 3, generator=_gen(cin + cout)) / math.sqrt(9 * cin))
        self.bias = nn.Parameter(torch.randn(cout, generator=_gen(cout))) if bias else None

    def forward(self, x):
        return self.pkg.ops.conv2d(x, self.weight, self.bias, 1, 1, precision=self.precision)


class _PwMod(nn.Module):
    def __init__(self, pkg):
        super().__init__()
        self.pkg = pkg
        self.weight = nn.Parameter(torch.randn(8, 8, 1, 1, generator=_gen(4)) / 3)

    def forward(self, x):
        return self.pkg.bf16.conv1x1(x, self.weight)


class Row(object):
    """One cache: make(pkg, dev) -> module (identical values each time), x(pkg, dev) -> input, mode: 'train' (forward + backward),
    'eval' (no_grad forward) or 'frozen' (eval-mode forward + backward); held(module) -> truthy once the cache is filled."""

    def __init__(self, attr, make, x, mode, held, fwd=None):
        self.attr, self.make, self.x, self.mode, self.held, self.fwd = attr, make, x, mode, held, fwd


def _pack_of(m, name='_ssg_pack'):
    c = m.weight.__dict__.get(name)
    return c[1] if c is not None else {}


def _rows():
    def conv_x(shape):
        return lambda pkg, dev: _nhwc(pkg, dev, torch.randn(*shape, generator=_gen(3)))
    x1x = conv_x((1, 32, 9, 17))
    return [
        Row('_ssg_pack', lambda pkg, dev: _ConvMod(pkg, 16, 32).to(dev), conv_x((2, 16, 20, 24)), 'train', lambda m: len(_pack_of(m)) >= 2),
        # tests/test_split_gpu.py's smallest k32 split shape (64 -> 64 channels at 48 x 64, batch 2)
        Row('_ssg_split', lambda pkg, dev: _ConvMod(pkg, 64, 64, bias=False).to(dev), conv_x((2, 64, 48, 64)), 'train',
            lambda m: any('_ssg_split' in t.__dict__ for t in _pack_of(m).values())),
        Row('_ssg_pack_bf16x1', lambda pkg, dev: _ConvMod(pkg, 32, 64, 'bf16x1').to(dev), x1x, 'train', lambda m: len(_pack_of(m, '_ssg_pack_bf16x1')) >= 1),
        Row('_ssg_pack_bf16x2', lambda pkg, dev: _ConvMod(pkg, 32, 64, 'bf16x2').to(dev), x1x, 'train', lambda m: len(_pack_of(m, '_ssg_pack_bf16x2')) >= 1),
        Row('_ssg_pack_bf16', lambda pkg, dev: _PwMod(pkg).to(dev),
            lambda pkg, dev: pkg.bf16.to_bf16(_nhwc(pkg, dev, torch.randn(1, 8, 10, 13, generator=_gen(5)))).detach(), 'train',
            lambda m: len(_pack_of(m, '_ssg_pack_bf16')) == 2),
        Row('_ssg_gb_cat', _make_spade, _spade_x, 'train', lambda m: '_ssg_gb_cat' in m.mlp_gamma.weight.__dict__, fwd=lambda m, x: m(x, x)),
        Row('_fold_cache', lambda pkg, dev: _make_block(pkg, dev, 'cached_eval'), conv_x((2, 16, 12, 13)), 'eval', lambda m: hasattr(m, '_fold_cache')),
        Row('_fold_consts_cache', lambda pkg, dev: _make_block(pkg, dev, 'frozen'), conv_x((2, 16, 12, 13)), 'frozen',
            lambda m: hasattr(m, '_fold_consts_cache') and hasattr(m, '_fold_cache')),
    ]


ROWS = OrderedDict((r.attr, r) for r in _rows())
# `_ssg_*` attributes that configure a module and cache nothing derived from a parameter
NOT_CACHES = {'_ssg_sync_group': 'process group of a synchronised batch norm', '_ssg_var_mode': 'variance formula of a batch norm',
              '_ssg_dtype': 'tensor family an EfficientNet was switched to', '_ssg_frozen': 'mark of batchnorm.freeze_batch_norm',
              '_ssg_pack_': 'prefix of the two bf16x1 / bf16x2 pack attributes'}
ELSEWHERE = {'_PLAN_CACHE': 'tests/test_step_tail_gpu.py (the optimizers\' launch plans)',
             '_GRAPHS': 'tests/test_infer_gpu.py::test_graph_replay_follows_load_state_dict'}


def test_every_cache_of_the_package_has_a_row(pkg):
    root = os.path.dirname(pkg.__file__)
    found = set()
    for d, _, files in os.walk(root):
        for f in files:
            if f.endswith('.py'):
                src = open(os.path.join(d, f)).read()
                found |= set(re.findall(r'_ssg_\w*', src))
                found |= set(re.findall(r'self\.(_\w*cache\w*)', src))
                found |= set(re.findall(r'^(_[A-Z_]*(?:CACHE|GRAPHS)[A-Z_]*) =', src, re.M))
    missing = found - set(ROWS) - set(NOT_CACHES) - set(ELSEWHERE)
    assert not missing, 'cache attributes without a row in the B2 grid: %s' % sorted(missing)
    assert set(ROWS) <= found and set(ELSEWHERE) <= found


def _row_run(row, m, x):
    fwd = row.fwd or (lambda m_, x_: m_(x_))
    m.zero_grad(set_to_none=True)
    res = OrderedDict()
    if row.mode == 'eval':
        with torch.no_grad():
            y = fwd(m, x)
    else:
        xg = x.detach().clone().requires_grad_(True) if x.dtype == torch.float32 else x.detach().requires_grad_(True)
        y = fwd(m, xg)
        y.backward(torch.randn(y.shape, generator=_gen(6)).to(y.dtype).to(y.device))
        res['dx'] = xg.grad
        for k, p in m.named_parameters():
            res['d:' + k] = p.grad
    res['y'] = y.detach().clone()
    torch.cuda.synchronize()
    return res


def _fresh(row, pkg, dev, m):
    """A module of the same construction holding clones of m's current values: none of its tensors ever held a cache."""
    f = row.make(pkg, dev)
    f.load_state_dict({k: v.detach().clone() for k, v in m.state_dict().items()})
    f.train(m.training)
    for a, b in zip(m.modules(), f.modules()):
        b.training = a.training
    for p in list(f.parameters()) + list(f.buffers()):
        assert not [k for k in p.__dict__ if k.startswith('_ssg_')]
    return f


def _grads(m):
    g = _gen(8)
    for p in m.parameters():
        p.grad = (torch.randn(p.shape, generator=g) * 0.1).to(p.device)


def _ev_mul(pkg, m, keep):
    with torch.no_grad():
        for p in m.parameters():
            p.mul_(1.5)


def _ev_load(pkg, m, keep):
    m.load_state_dict({k: (v * 0.75 + 0.0625 if v.is_floating_point() else v) for k, v in m.state_dict().items()})


def _ev_sgd(pkg, m, keep):
    _grads(m)
    torch.optim.SGD(m.parameters(), lr=0.1).step()


def _ev_fused_adam(pkg, m, keep):
    _grads(m)
    pkg.optim.clip_adam_step(torch.optim.Adam(m.parameters(), lr=1e-2), 0.05)


def _ev_fused_sgd(pkg, m, keep):
    _grads(m)
    pkg.optim.clip_sgd_step(torch.optim.SGD(m.parameters(), lr=0.1, momentum=0.9), 0.05)


def _ev_clamp(pkg, m, keep):
    pkg.optim.clamp_parameters_(list(m.parameters()), 0.02)


def _ev_data(pkg, m, keep):
    for p in m.parameters():
        keep.append(p.data)                         # the old storage stays alive: the new one cannot get its address
        p.data = p.data * 1.25 + 0.03125


def _ev_train_forward(pkg, m, keep):
    was = [(mod, mod.training) for mod in m.modules()]
    m.train()
    m(keep['x'])
    for mod, t in was:
        mod.training = t


def _ev_fill_var(pkg, m, keep):
    m.bn2.running_var.fill_(2.0)


def _ev_bn_weight(pkg, m, keep):
    with torch.no_grad():
        m.bn1.weight.add_(0.5)


EVENTS = OrderedDict([('mul_', _ev_mul), ('load_state_dict', _ev_load), ('torch-sgd', _ev_sgd), ('fused-adam', _ev_fused_adam),
                      ('fused-sgd', _ev_fused_sgd), ('clamp', _ev_clamp), ('data=', _ev_data)])
FOLD_EVENTS = OrderedDict([('train-forward', _ev_train_forward), ('running_var.fill_', _ev_fill_var), ('bn.weight', _ev_bn_weight)])
GRID = [(a, e) for a in ROWS for e in EVENTS] + [(a, e) for a in ('_fold_cache', '_fold_consts_cache') for e in FOLD_EVENTS]


class _Keep(dict):
    def append(self, v):
        self.setdefault('old', []).append(v)


@pytest.mark.parametrize('attr,event', GRID, ids=['%s-%s' % g for g in GRID])
def test_b2_cache_follows_event(pkg, dev, attr, event):
    row = ROWS[attr]
    m, x = row.make(pkg, dev), row.x(pkg, dev)
    r0 = _row_run(row, m, x)
    assert row.held(m), '%s: the warm forward did not fill the cache (wrong route for this row)' % attr
    r1 = _row_run(row, m, x)
    exact = all(torch.equal(r0[k], r1[k]) for k in r0)
    if not exact:
        print('tolerance branch: cache row %s is not run-to-run reproducible' % attr)
    keep = _Keep(x=x)
    before = [p.detach().clone() for p in list(m.parameters()) + list(m.buffers())]
    dict(EVENTS, **FOLD_EVENTS)[event](pkg, m, keep)
    after = list(m.parameters()) + list(m.buffers())
    assert any(not torch.equal(a, b) for a, b in zip(before, after)), 'the event changed nothing'
    got = _row_run(row, m, x)
    ref = _row_run(row, _fresh(row, pkg, dev, m), x)
    assert not torch.equal(ref['y'], r0['y']), 'the event did not move the output: the cell would pass on a stale cache'
    # tests/test_blocks_gpu.py::_check / test_conv2d_fwd_bwd's weight gradient bound for the tolerance branch
    _same(got, ref, exact, (1e-4, 1e-4), '%s after %s' % (attr, event))


def test_b2_raw_write_needs_a_bump(pkg, dev):
    """The documented limitation: a write through .data is invisible to the stamp until bump_weight_epoch()."""
    row = ROWS['_ssg_pack']
    m, x = row.make(pkg, dev), row.x(pkg, dev)
    with torch.no_grad():
        y0 = m(x).clone()
        m.weight.data.mul_(2.0)
        assert torch.equal(m(x), y0)
        pkg.ops.bump_weight_epoch()
        y2 = m(x).clone()
        ref = _fresh(row, pkg, dev, m)(x)
    assert not torch.equal(y2, y0) and torch.equal(y2, ref)


def test_b2_precision_switch_keeps_each_family_apart(pkg, dev):
    m, x = _ConvMod(pkg, 32, 64).to(dev), ROWS['_ssg_pack_bf16x1'].x(pkg, dev)
    first = {}
    with torch.no_grad():
        for lap in range(2):
            for prec in ('fp32', 'bf16x1', 'bf16x2', 'fp32'):
                m.precision = prec
                y = m(x).clone()
                assert torch.equal(first.setdefault(prec, y), y), (lap, prec)
    assert not torch.equal(first['fp32'], first['bf16x1']) and not torch.equal(first['bf16x1'], first['bf16x2'])
    assert _pack_of(m, '_ssg_pack_bf16x1') and _pack_of(m, '_ssg_pack_bf16x2') and _pack_of(m)


def test_b2_shared_weight_is_seen_by_both_modules(pkg, dev):
    a = _ConvMod(pkg, 16, 32).to(dev)
    b = _ConvMod(pkg, 16, 32, weight=a.weight).to(dev)
    x = ROWS['_ssg_pack'].x(pkg, dev)
    with torch.no_grad():
        ya0, yb0 = a(x).clone(), b(x).clone()
        a.weight.mul_(1.5)
        ya1, yb1 = a(x).clone(), b(x).clone()
        fa = _ConvMod(pkg, 16, 32).to(dev); fa.load_state_dict({k: v.clone() for k, v in a.state_dict().items()})
        fb = _ConvMod(pkg, 16, 32).to(dev); fb.load_state_dict({k: v.clone() for k, v in b.state_dict().items()})
        assert torch.equal(ya1, fa(x)) and torch.equal(yb1, fb(x))
    assert b.weight is a.weight and not torch.equal(ya1, ya0) and not torch.equal(yb1, yb0)
