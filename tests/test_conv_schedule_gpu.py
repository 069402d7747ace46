"""The ordered ops.PROFILE label list of one forward + backward, for every schedule that decides which conv kernels run and in which
order: archs.BasicBlock train-mode and frozen (blocks._BasicBlockFn / _FrozenBasicBlockFn) without a context and under
ops.train_precision('bf16x1'), with and without the two off-by-default batch-norm fusions; ops.conv2d and ops.conv2d_bf16x1_train;
blocks.spade_self.  A label depends only on the shapes, so each list is a literal: EXPECTED was printed by print_expected() on the
commit BEFORE the conv launch path of ops.py was unified, and pasted in.  It pins every launch and its position; the values are
pinned elsewhere (tests/test_train_x1_gpu.py, tests/test_blocks_gpu.py, tests/test_frozen_block_gpu.py)."""
import contextlib
import pprint

import pytest
import torch
import torch.nn as nn

import train_x1_ref as tr

# block cases: train_x1_ref.CASES, and a 16-pixel-wide block on which every bf16x1 predicate refuses
W16 = (2, 64, 0, 64, 8, 16)


def _tensors(*ts):
    return [t.detach().cpu() for t in ts if t is not None]


def _block(pkg, dev, case, mode, precision, flag=None):
    if case == 'w16':
        n, c1, c2, planes, h, w = W16
        g = torch.Generator().manual_seed(9)
        x1 = torch.randn(n, c1, h, w, generator=g); x2 = None; dout = torch.randn(n, planes, h, w, generator=g)
        torch.manual_seed(3)
        blk = pkg.archs.BasicBlock(c1, planes)
    else:
        st, x1, x2, dout = tr.make_case(case)
        n, c1, c2, planes, h, w = tr.CASES[case]
        blk = pkg.archs.BasicBlock(c1 + c2, planes)
        if 'shortcut.0.weight' in st and not len(blk.shortcut):
            blk.shortcut = nn.Sequential(nn.Conv2d(c1 + c2, planes, kernel_size=1, bias=False))
        sd = blk.state_dict(); sd.update({k: v.clone() for k, v in st.items()})
        blk.load_state_dict(sd)
    blk.to(dev).train()
    if mode == 'frozen':
        blk.bn1.eval(); blk.bn2.eval()
    assert blk._route() == mode
    a = x1.to(dev).requires_grad_(True)
    b = x2.to(dev).requires_grad_(True) if x2 is not None else None
    ops = pkg.ops
    saved = (ops.BN_FUSE_INPUT, ops.BN_BWD_EPILOGUE)
    try:
        if flag is not None:
            setattr(ops, flag, True)
        with ops.train_precision(precision) if precision else contextlib.nullcontext():
            out = blk(a, b)
            out.backward(dout.to(dev))
    finally:
        ops.BN_FUSE_INPUT, ops.BN_BWD_EPILOGUE = saved
    return _tensors(out, a.grad, b.grad if b is not None else None, *[p.grad for p in blk.parameters()])


def _block_stride2(pkg, dev, precision):
    """1 x 64 -> 128 on 16 x 36, stride 2: only w1 and the shortcut weight require grad (there is no strided input gradient)."""
    torch.manual_seed(5)
    blk = pkg.archs.BasicBlock(64, 128, stride=2).to(dev).train()
    for name, p in blk.named_parameters():
        p.requires_grad_(name in ('conv1.weight', 'shortcut.0.weight'))
    g = torch.Generator().manual_seed(6)
    x = torch.randn(1, 64, 16, 36, generator=g).to(dev); dout = torch.randn(1, 128, 8, 18, generator=g).to(dev)
    with pkg.ops.train_precision(precision) if precision else contextlib.nullcontext():
        out = blk(x)
        out.backward(dout)
    return _tensors(out, blk.conv1.weight.grad, blk.shortcut[0].weight.grad)


def _conv(pkg, dev, x1_train):
    """act(conv3x3(cat(x, x2)) + bias + res), ReLU, 2 x (64 + 64) -> 128 on 6 x 33: ops.conv2d, or ops.conv2d_bf16x1_train."""
    ops = pkg.ops
    g = torch.Generator().manual_seed(23)
    n, c1, c2, co, h, w = 2, 64, 64, 128, 6, 33
    host = [torch.randn(n, c1, h, w, generator=g), torch.randn(n, c2, h, w, generator=g),
            torch.randn(co, c1 + c2, 3, 3, generator=g) / (3 * (c1 + c2) ** 0.5), torch.randn(co, generator=g) * 0.2,
            torch.randn(n, co, h, w, generator=g)]
    dout = torch.randn(n, co, h, w, generator=g).to(dev)
    x, x2, wt, bias, res = [t.to(dev).requires_grad_(True) for t in host]
    if x1_train:
        y = ops.conv2d_bf16x1_train(x, wt, bias, act=1, x2=x2, res=res)
    else:
        y = ops.conv2d(x, wt, bias, 1, 1, act=1, x2=x2, res=res)
    y.backward(dout)
    return _tensors(y, x.grad, x2.grad, wt.grad, bias.grad, res.grad)


def _conv_stride2(pkg, dev):
    """3x3 stride-2 conv 1 x 64 -> 64 on 16 x 36 with an input gradient: the four parity classes as one launch."""
    g = torch.Generator().manual_seed(29)
    x = torch.randn(1, 64, 16, 36, generator=g).to(dev).requires_grad_(True)
    wt = (torch.randn(64, 64, 3, 3, generator=g) / 24).to(dev).requires_grad_(True)
    y = pkg.ops.conv2d(x, wt, None, 2, 1)
    y.backward(torch.randn(1, 64, 8, 18, generator=g).to(dev))
    return _tensors(y, x.grad, wt.grad)


def _spade(pkg, dev):
    """blocks.spade_self at 1 x 64 channels on 20 x 20: too few pixels for the fused gamma|beta kernel."""
    torch.manual_seed(12)
    m = pkg.normalization.SPADE('spadebatch3x3', 64, 3, 4).to(dev).train()
    g = torch.Generator().manual_seed(31)
    x = torch.randn(1, 64, 20, 20, generator=g).to(dev).requires_grad_(True)
    y = pkg.blocks.spade_self(x, m.x2map, m.mlp_shared[0], m.mlp_gamma, m.mlp_beta)
    y.backward(torch.randn(1, 64, 20, 20, generator=g).to(dev))
    return _tensors(y, x.grad, *[p.grad for p in m.parameters()])


def _cases():
    c = {}
    for mode in ('train', 'frozen'):
        for case in ('id64', 'cat128', 'w16'):
            for precision in (None, 'bf16x1'):
                c['block-%s-%s-%s' % (mode, case, precision or 'none')] = \
                    lambda pkg, dev, a=(case, mode, precision): _block(pkg, dev, *a)
    for precision in (None, 'bf16x1'):
        c['block-train-stride2-%s' % (precision or 'none')] = lambda pkg, dev, p=precision: _block_stride2(pkg, dev, p)
    c['conv2d'] = lambda pkg, dev: _conv(pkg, dev, False)
    c['conv2d_bf16x1_train'] = lambda pkg, dev: _conv(pkg, dev, True)
    c['conv2d-stride2'] = _conv_stride2
    c['spade_self'] = _spade
    for flag in ('BN_FUSE_INPUT', 'BN_BWD_EPILOGUE'):
        for precision in (None, 'bf16x1'):
            c['block-train-cat128-%s-%s' % (precision or 'none', flag)] = \
                lambda pkg, dev, a=('cat128', 'train', precision, flag): _block(pkg, dev, *a)
    return c


CASES = _cases()


def record(pkg, dev, name):
    """(labels, tensors) of CASES[name]: the ordered ops.PROFILE labels of its forward + backward, and what it computed."""
    pkg.ops.PROFILE = []
    try:
        got = CASES[name](pkg, dev)
        torch.cuda.synchronize()
        return [rec[0] for rec in pkg.ops.PROFILE], got
    finally:
        pkg.ops.PROFILE = None


def print_expected(pkg, dev):
    """Prints the EXPECTED literal below (run on a commit whose schedule is the one to pin)."""
    print('EXPECTED = ' + pprint.pformat({name: record(pkg, dev, name)[0] for name in CASES}, width=130, sort_dicts=False, compact=True))


EXPECTED = {'block-train-id64-none': ['conv_igemm_halo_x3_kernel<128,64>', 'conv_igemm_halo_x3_kernel<128,64>', 'wgrad_k32_kernel<64,64>',
                           'conv_igemm_halo_x3_kernel<128,64>', 'wgrad_k32_kernel<64,64>', 'conv_igemm_halo_x3_kernel<128,64>'],
 'block-train-id64-bf16x1': ['conv_halo_k32_x1_kernel<64>', 'conv_halo_k32_x1_kernel<64>', 'wgrad_k32_x1_kernel',
                             'conv_halo_k32_x1_kernel<64>', 'wgrad_k32_x1_kernel', 'conv_halo_k32_x1_kernel<64>'],
 'block-train-cat128-none': ['conv_igemm_halo_kernel<128,64>+splitk', 'conv_igemm_halo_kernel<128,64>+splitk',
                             'conv_igemm_dma_kernel<128,64>', 'wgrad_k32_kernel<64,64>', 'conv_igemm_halo_kernel<128,64>+splitk',
                             'wgrad_k32_kernel<64,64>', 'wgrad_dma_x3_kernel<128,128>', 'conv_igemm_dma_kernel<128,64>',
                             'conv_igemm_halo_kernel<128,64>+splitk', 'conv_igemm_dma_kernel<128,64>',
                             'conv_igemm_halo_kernel<128,64>+splitk'],
 'block-train-cat128-bf16x1': ['conv_halo_k32_x1_kernel<128>', 'conv_halo_k32_x1_kernel<128>', 'conv_igemm_dma_kernel<128,64>',
                               'wgrad_k32_x1_kernel', 'conv_halo_k32_x1_kernel<128>', 'wgrad_k32_x1_kernel',
                               'wgrad_dma_x3_kernel<128,128>', 'conv_igemm_dma_kernel<128,64>', 'conv_halo_k32_x1_kernel<64>',
                               'conv_igemm_dma_kernel<128,64>', 'conv_halo_k32_x1_kernel<64>'],
 'block-train-w16-none': ['conv_igemm_halo16_kernel<128,64>', 'conv_igemm_halo16_kernel<128,64>', 'wgrad_halo_x3_kernel<64,64>',
                          'conv_igemm_halo16_kernel<128,64>', 'wgrad_halo_x3_kernel<64,64>', 'conv_igemm_halo16_kernel<128,64>'],
 'block-train-w16-bf16x1': ['conv_igemm_halo16_kernel<128,64>', 'conv_igemm_halo16_kernel<128,64>', 'wgrad_halo_x3_kernel<64,64>',
                            'conv_igemm_halo16_kernel<128,64>', 'wgrad_halo_x3_kernel<64,64>',
                            'conv_igemm_halo16_kernel<128,64>'],
 'block-frozen-id64-none': ['conv_igemm_halo_x3_kernel<128,64>', 'conv_igemm_halo_x3_kernel<128,64>', 'wgrad_k32_kernel<64,64>',
                            'conv_igemm_halo_x3_kernel<128,64>', 'wgrad_k32_kernel<64,64>', 'conv_igemm_halo_x3_kernel<128,64>'],
 'block-frozen-id64-bf16x1': ['conv_halo_k32_x1_kernel<64>', 'conv_halo_k32_x1_kernel<64>', 'wgrad_k32_x1_kernel',
                              'conv_halo_k32_x1_kernel<64>', 'wgrad_k32_x1_kernel', 'conv_halo_k32_x1_kernel<64>'],
 'block-frozen-cat128-none': ['conv_igemm_halo_kernel<128,64>+splitk', 'conv_igemm_dma_kernel<128,64>',
                              'conv_igemm_halo_kernel<128,64>+splitk', 'wgrad_k32_kernel<64,64>', 'wgrad_dma_x3_kernel<128,128>',
                              'conv_igemm_halo_kernel<128,64>+splitk', 'wgrad_k32_kernel<64,64>', 'conv_igemm_dma_kernel<128,64>',
                              'conv_igemm_halo_kernel<128,64>+splitk', 'conv_igemm_dma_kernel<128,64>',
                              'conv_igemm_halo_kernel<128,64>+splitk'],
 'block-frozen-cat128-bf16x1': ['conv_halo_k32_x1_kernel<128>', 'conv_igemm_dma_kernel<128,64>', 'conv_halo_k32_x1_kernel<128>',
                                'wgrad_k32_x1_kernel', 'wgrad_dma_x3_kernel<128,128>', 'conv_halo_k32_x1_kernel<128>',
                                'wgrad_k32_x1_kernel', 'conv_igemm_dma_kernel<128,64>', 'conv_halo_k32_x1_kernel<64>',
                                'conv_igemm_dma_kernel<128,64>', 'conv_halo_k32_x1_kernel<64>'],
 'block-frozen-w16-none': ['conv_igemm_halo16_kernel<128,64>', 'conv_igemm_halo16_kernel<128,64>', 'wgrad_halo_x3_kernel<64,64>',
                           'conv_igemm_halo16_kernel<128,64>', 'wgrad_halo_x3_kernel<64,64>',
                           'conv_igemm_halo16_kernel<128,64>'],
 'block-frozen-w16-bf16x1': ['conv_igemm_halo16_kernel<128,64>', 'conv_igemm_halo16_kernel<128,64>',
                             'wgrad_halo_x3_kernel<64,64>', 'conv_igemm_halo16_kernel<128,64>', 'wgrad_halo_x3_kernel<64,64>',
                             'conv_igemm_halo16_kernel<128,64>'],
 'block-train-stride2-none': ['conv_igemm_dma_kernel<128,128>', 'conv_igemm_halo_kernel<128,64>+splitk',
                              'conv_igemm_dma_kernel<128,64>', 'wgrad_k32_kernel<64,64>', 'conv_igemm_halo_kernel<128,64>+splitk',
                              'wgrad_dma_x3_kernel<128,128>', 'wgrad_dma_x3_kernel<128,128>'],
 'block-train-stride2-bf16x1': ['conv_igemm_dma_kernel<128,128>', 'conv_igemm_halo_kernel<128,64>+splitk',
                                'conv_igemm_dma_kernel<128,64>', 'wgrad_k32_kernel<64,64>',
                                'conv_igemm_halo_kernel<128,64>+splitk', 'wgrad_dma_x3_kernel<128,128>',
                                'wgrad_dma_x3_kernel<128,128>'],
 'conv2d': ['conv_igemm_halo_kernel<128,64>+splitk', 'conv_igemm_halo_kernel<128,64>+splitk',
            'conv_igemm_halo_kernel<128,64>+splitk', 'wgrad_k32_kernel<64,64>'],
 'conv2d_bf16x1_train': ['conv_halo_k32_x1_kernel<128>', 'conv_halo_k32_x1_kernel<64>', 'conv_halo_k32_x1_kernel<64>',
                         'wgrad_k32_x1_kernel'],
 'conv2d-stride2': ['conv_igemm_dma_kernel<256,64>', 'conv_igemm_halo_x3_kernel<128,64,4,1,true>', 'wgrad_dma_x3_kernel<128,64>'],
 'spade_self': ['thin4_cout_kernel', 'tiny4_kernel', 'thin4_cin_kernel', 'wgrad4_kernel<thin_cin>', 'thin4_cout_kernel',
                'wgrad_tiny4_kernel', 'tiny4_kernel', 'wgrad4_kernel<thin_cout>', 'thin4_cin_kernel'],
 'block-train-cat128-none-BN_FUSE_INPUT': ['conv_igemm_halo_kernel<128,64>+splitk', 'conv_igemm_halo_kernel<128,64>+splitk',
                                           'conv_igemm_dma_kernel<128,64>', 'wgrad_k32_kernel<64,64>',
                                           'conv_igemm_halo_kernel<128,64>+splitk', 'wgrad_k32_kernel<64,64>',
                                           'wgrad_dma_x3_kernel<128,128>', 'conv_igemm_dma_kernel<128,64>',
                                           'conv_igemm_halo_kernel<128,64>+splitk', 'conv_igemm_dma_kernel<128,64>',
                                           'conv_igemm_halo_kernel<128,64>+splitk'],
 'block-train-cat128-bf16x1-BN_FUSE_INPUT': ['conv_halo_k32_x1_kernel<128>', 'conv_halo_k32_x1_kernel<128>',
                                             'conv_igemm_dma_kernel<128,64>', 'wgrad_k32_x1_kernel',
                                             'conv_halo_k32_x1_kernel<128>', 'wgrad_k32_x1_kernel',
                                             'wgrad_dma_x3_kernel<128,128>', 'conv_igemm_dma_kernel<128,64>',
                                             'conv_halo_k32_x1_kernel<64>', 'conv_igemm_dma_kernel<128,64>',
                                             'conv_halo_k32_x1_kernel<64>'],
 'block-train-cat128-none-BN_BWD_EPILOGUE': ['conv_igemm_halo_kernel<128,64>+splitk', 'conv_igemm_halo_kernel<128,64>+splitk',
                                             'conv_igemm_dma_kernel<128,64>', 'wgrad_k32_kernel<64,64>',
                                             'conv_igemm_halo_kernel<128,64>+splitk', 'wgrad_k32_kernel<64,64>',
                                             'wgrad_dma_x3_kernel<128,128>', 'conv_igemm_dma_kernel<128,64>',
                                             'conv_igemm_halo_kernel<128,64>+splitk', 'conv_igemm_dma_kernel<128,64>',
                                             'conv_igemm_halo_kernel<128,64>+splitk'],
 'block-train-cat128-bf16x1-BN_BWD_EPILOGUE': ['conv_halo_k32_x1_kernel<128>', 'conv_halo_k32_x1_kernel<128>',
                                               'conv_igemm_dma_kernel<128,64>', 'wgrad_k32_x1_kernel',
                                               'conv_halo_k32_x1_kernel<128>', 'wgrad_k32_x1_kernel',
                                               'wgrad_dma_x3_kernel<128,128>', 'conv_igemm_dma_kernel<128,64>',
                                               'conv_halo_k32_x1_kernel<64>', 'conv_igemm_dma_kernel<128,64>',
                                               'conv_halo_k32_x1_kernel<64>']}


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(CASES))
def test_label_list(pkg, dev, name):
    labels, _ = record(pkg, dev, name)
    assert labels == EXPECTED[name], labels


def test_expected_lists_relate_as_the_routing_rules_say():
    E = EXPECTED
    assert set(E) == set(CASES)
    for mode in ('train', 'frozen'):
        # every bf16x1 launch refused (16 pixels wide): the fp32 list
        assert E['block-%s-w16-bf16x1' % mode] == E['block-%s-w16-none' % mode]
        for case in ('id64', 'cat128'):
            assert E['block-%s-%s-bf16x1' % (mode, case)] != E['block-%s-%s-none' % (mode, case)]
    # a stride-2 block never reads the mode
    assert E['block-train-stride2-bf16x1'] == E['block-train-stride2-none']
    # the two batch-norm fusions stay off under bf16x1
    for flag in ('BN_FUSE_INPUT', 'BN_BWD_EPILOGUE'):
        assert E['block-train-cat128-bf16x1-%s' % flag] == E['block-train-cat128-bf16x1']
