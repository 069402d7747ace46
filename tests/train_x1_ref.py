"""A quantised fp64 BasicBlock, train mode and frozen, in plain torch on the CPU: the reference for ops.train_precision('bf16x1')
(blocks._BasicBlockFn / _FrozenBasicBlockFn on csrc/conv_halo_k32_bf16.hip and csrc/conv_wgrad_k32_bf16.hip).  Plain helper module
(not a conftest); nothing here calls an op under test.

The block rounds to bf16 (bn_ref.bf16_rne) exactly where the kernels do, and nowhere else:

    site   launch                         operands rounded
    f1     conv1 forward                  x = cat(x1, x2) and w1 (the FOLDED weight on the frozen route)
    f2     conv2 forward                  y1 and w2
    d2     input gradient of conv2        dy and w2
    d1     input gradient of conv1        dy and w1
    w2     weight gradient of conv2       y1 and dy
    w1     weight gradient of conv1       x and dy

each as two sites ('f1x', 'f1w', ..., 'w1x', 'w1dy').  The 1x1 shortcut, both batch norms (batch statistics or the fold), the
ReLUs, every sum and the residual are fp64 and unrounded.  `sites` = the set of active sites: ALL is the device's routing, the
empty set the unquantised block; the rehearsal removes one site or adds one at the shortcut ('scx', 'scw', 'scdy').

stats(case, mode): per gradient (x1, x2, w1, w2, wsc, g1, b1, g2, b2) and for the block's output the (max, RMS) error of the
quantised block against the unquantised one, both with the same ReLU masks imposed.  The device's error against the unquantised
block (under the device's masks) may be at most MAX_MARGIN x / RMS_MARGIN x that, or the fp32-class floor where no rounding site
reaches a tensor (wsc and b2: their statistic is exactly zero)."""
import numpy as np
import torch
import torch.nn.functional as F

from bn_ref import bf16_rne

ALL = frozenset(['f1x', 'f1w', 'f2x', 'f2w', 'd2dy', 'd2w', 'd1dy', 'd1w', 'w2x', 'w2dy', 'w1x', 'w1dy'])
SHORTCUT_SITES = ('scx', 'scw', 'scdy')
MAX_MARGIN, RMS_MARGIN = 1.5, 1.25
EPS = 1e-5

# (N, C1, C2, planes, H, W): an identity-shortcut block, and the two-pointer decoder block with the 1x1 shortcut on an odd width
# (a full 32-pixel strip plus one pixel)
CASES = {'id64': (2, 64, 0, 64, 8, 24), 'cat128': (2, 64, 64, 128, 6, 33)}
GRADS = ('x1', 'x2', 'w1', 'w2', 'wsc', 'g1', 'b1', 'g2', 'b2')
PARAM_OF = {'w1': 'conv1.weight', 'w2': 'conv2.weight', 'wsc': 'shortcut.0.weight', 'g1': 'bn1.weight', 'b1': 'bn1.bias',
            'g2': 'bn2.weight', 'b2': 'bn2.bias'}


def q(t):
    """fp64 tensor -> its fp32 value rounded to bf16 (nearest even), as fp64."""
    return torch.from_numpy(bf16_rne(t.detach().float().numpy()).astype(np.float64))


def make_case(name, seed=17):
    """(state, x1, x2, dout): fp32 CPU tensors.  state = the BasicBlock's parameters and running statistics by state_dict name."""
    n, c1, c2, planes, h, w = CASES[name]
    g = torch.Generator().manual_seed(seed + sum(CASES[name]))
    cin = c1 + c2
    st = {'conv1.weight': torch.randn(planes, cin, 3, 3, generator=g) / (3 * cin ** 0.5),
          'conv2.weight': torch.randn(planes, planes, 3, 3, generator=g) / (3 * planes ** 0.5)}
    if cin != planes or c2:                  # a two-tensor input has no identity shortcut: the 1x1 conv
        st['shortcut.0.weight'] = torch.randn(planes, cin, 1, 1, generator=g) / cin ** 0.5
    for bn in ('bn1', 'bn2'):
        st[bn + '.weight'] = torch.rand(planes, generator=g) + 0.5
        st[bn + '.bias'] = torch.randn(planes, generator=g) * 0.2
        st[bn + '.running_mean'] = torch.randn(planes, generator=g) * 0.1
        st[bn + '.running_var'] = torch.rand(planes, generator=g) * 0.5 + 0.25
    x1 = torch.randn(n, c1, h, w, generator=g)
    x2 = torch.randn(n, c2, h, w, generator=g) if c2 else None
    dout = torch.randn(n, planes, h, w, generator=g)
    return st, x1, x2, dout


class _QConv(torch.autograd.Function):
    """conv3x3 (pad 1, stride 1) in fp64 whose three launches round their operands at the sites named in `sites` with prefix
    f / d / w + `k` (k = '1' or '2')."""

    @staticmethod
    def forward(ctx, x, w, k, sites):
        ctx.save_for_backward(x, w)
        ctx.k, ctx.sites = k, sites
        xf = q(x) if 'f%sx' % k in sites else x
        wf = q(w) if 'f%sw' % k in sites else w
        return F.conv2d(xf, wf, None, 1, 1)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        k, sites = ctx.k, ctx.sites
        dyd = q(dy) if 'd%sdy' % k in sites else dy
        wd = q(w) if 'd%sw' % k in sites else w
        dx = torch.nn.grad.conv2d_input(x.shape, wd, dyd, stride=1, padding=1)
        xw = q(x) if 'w%sx' % k in sites else x
        dyw = q(dy) if 'w%sdy' % k in sites else dy
        dw = torch.nn.grad.conv2d_weight(xw, w.shape, dyw, stride=1, padding=1)
        return dx, dw, None, None


class _QConv1x1(torch.autograd.Function):
    """The 1x1 shortcut; rounds only under the planted defects 'scx' / 'scw' (forward operands) and 'scdy' (both gradients' dy)."""

    @staticmethod
    def forward(ctx, x, w, sites):
        ctx.save_for_backward(x, w)
        ctx.sites = sites
        return F.conv2d(q(x) if 'scx' in sites else x, q(w) if 'scw' in sites else w)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        if 'scdy' in ctx.sites:
            dy = q(dy)
        return torch.nn.grad.conv2d_input(x.shape, w, dy), torch.nn.grad.conv2d_weight(x, w.shape, dy), None


def _relu(z, masks, i):
    return F.relu(z) if masks is None else torch.where(masks[i], z, torch.zeros_like(z))


def block(case, mode, sites, masks=None, with_out=False):
    """Gradients {name: fp64 tensor} and (y1 > 0, out > 0) of the block of make_case(case) in `mode` ('train': batch statistics,
    'frozen': running statistics folded into the conv weights, the folded weight being what is rounded).  masks = (m1, m2):
    the two ReLUs pass exactly these elements (imposed), None: their own."""
    st, x1, x2, dout = make_case(case)
    P = {k: v.double().requires_grad_(k.endswith(('weight', 'bias'))) for k, v in st.items()}
    a = x1.double().requires_grad_(True)
    b = x2.double().requires_grad_(True) if x2 is not None else None
    x = a if b is None else torch.cat([a, b], 1)
    sites = frozenset(sites)
    if mode == 'train':
        z1 = F.batch_norm(_QConv.apply(x, P['conv1.weight'], '1', sites), None, None, P['bn1.weight'], P['bn1.bias'], True, 0.0, EPS)
        y1 = _relu(z1, masks, 0)
        z2 = F.batch_norm(_QConv.apply(y1, P['conv2.weight'], '2', sites), None, None, P['bn2.weight'], P['bn2.bias'], True, 0.0, EPS)
    else:
        def fold(conv, bn):
            s = P[bn + '.weight'] * torch.rsqrt(P[bn + '.running_var'] + EPS)
            return P[conv + '.weight'] * s.view(-1, 1, 1, 1), P[bn + '.bias'] - P[bn + '.running_mean'] * s
        wf1, bf1 = fold('conv1', 'bn1')
        wf2, bf2 = fold('conv2', 'bn2')
        y1 = _relu(_QConv.apply(x, wf1, '1', sites) + bf1.view(1, -1, 1, 1), masks, 0)
        z2 = _QConv.apply(y1, wf2, '2', sites) + bf2.view(1, -1, 1, 1)
    r = _QConv1x1.apply(x, P['shortcut.0.weight'], sites) if 'shortcut.0.weight' in P else x
    out = _relu(z2 + r, masks, 1)
    out.backward(dout.double())
    grads = {'x1': a.grad, 'x2': b.grad if b is not None else None}
    for k, pk in PARAM_OF.items():
        grads[k] = P[pk].grad if pk in P else None
    grads = {k: v for k, v in grads.items() if v is not None}
    m = (y1.detach() > 0, out.detach() > 0)
    return (grads, m, out.detach()) if with_out else (grads, m)


def maxrms(e):
    e = e.double().abs()
    return e.max().item(), e.pow(2).mean().sqrt().item()


LAUNCHES = {'f1': ('f1x', 'f1w'), 'f2': ('f2x', 'f2w'), 'd2': ('d2dy', 'd2w'), 'd1': ('d1dy', 'd1w'), 'w2': ('w2x', 'w2dy'), 'w1': ('w1x', 'w1dy')}
_CACHE = {}


def own_masks(case, mode):
    """The ReLU masks of the quantised block (all sites): what the device's masks are, up to ties."""
    key = (case, mode, 'masks')
    if key not in _CACHE:
        _CACHE[key] = block(case, mode, ALL)[1]
    return _CACHE[key]


def tensors(case, mode, sites, masks):
    """{name: fp64 tensor}: the gradients and 'out', the block's output, under the imposed masks."""
    g, _, out = block(case, mode, sites, masks, with_out=True)
    g = dict(g); g['out'] = out
    return g


def stats(case, mode, sites=ALL, masks=None):
    """{tensor: (max, RMS, max|T|)}: the error of the block with `sites` against the unquantised block, both under the same imposed
    ReLU masks (None: own_masks), and the unquantised tensor's largest magnitude.  A ReLU that flips moves a gradient by O(1) at
    one element, which would drown the rounding statistics; with the masks imposed the statistic is the roundings' alone."""
    masks = own_masks(case, mode) if masks is None else masks
    ref = tensors(case, mode, frozenset(), masks)
    got = tensors(case, mode, sites, masks)
    return {k: maxrms(got[k] - ref[k]) + (ref[k].abs().max().item(),) for k in ref}
