"""Flip / rotation test-time augmentation on the device (csrc/sw_tta.hip): the oriented gather against torch.rot90 /
torch.flip of the unoriented one, the reduce against its torch restatement, `segment_image(tta=...)` against the loop it stands
for.  Every step is a move, an fp32 add in a fixed order or a scaling by a power of two, so every comparison is torch.equal /
np.array_equal -- no tolerance."""
import numpy as np
import pytest
import torch

import tta_ref as R
from test_sw_labels_host import label_image

SETS = ('hflip', 'flips', 'd4')


def _cfg(p_size, size, classes=3):
    return dict(patch_size=p_size, input_w=size, input_h=size, patch_overlap=0.5, num_classes=classes)


def _image(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _raw(x):
    """The [N, H, W, ld] memory behind an NHWC tensor, pad lanes included (a view: writes reach the tensor)."""
    n, c, h, w = x.shape
    ld = x.stride(3) if w > 1 else 4 * ((c + 3) // 4)
    return torch.empty(0, dtype=x.dtype, device=x.device).set_(x.untyped_storage(), x.storage_offset(), (n, h, w, ld), (h * w * ld, w * ld, ld, 1))


# ----------------------------------------------------------------------------- [9] the oriented gather
@pytest.mark.gpu
@pytest.mark.parametrize('factor', [1, 2])
@pytest.mark.parametrize('size', [8, 40, 64])
def test_oriented_gather_is_the_view_of_the_unoriented_gather(pkg, dev, size, factor):
    ops = pkg.ops
    h, w, p = 200, 136, size * factor
    img = torch.from_numpy(_image(h, w, 70)).to(dev)
    corners = [(0, 0), (0, w - p), (h - p, 0), (h - p, w - p)]
    for org in ([(h - p, w - p)], corners + [((h - p) // 2 + 1, (w - p) // 2 + 1)]):      # P = 1 and P = 5
        base = ops.sw_gather_patches(img, org, p, size)
        assert torch.equal(base, ops.sw_gather_patches(img, org, p, size, orient=0))
        seen = set()
        for k in range(8):
            got = ops.sw_gather_patches(img, org, p, size, orient=k)
            assert tuple(got.shape) == (len(org), 3, size, size) and ops.nhwc_ld(got) == 4
            assert torch.equal(got, R.T_t(base, k)), (len(org), k)
            assert not _raw(got)[..., 3].view(torch.int32).any()                 # pad lane: +0.0 exactly
            seen.add(got.cpu().numpy().tobytes())
        assert len(seen) == 8                                                    # a random image has no symmetry: 8 different answers


# ----------------------------------------------------------------------------- [10] the reduce
CODE_LISTS = {1: [(k,) for k in range(8)], 2: [(5, 2), (3, 0), (4, 7), (6, 1)], 4: [(6, 1, 4, 3), (0, 2, 5, 7), (7, 5, 3, 1)],
              8: [(3, 6, 0, 5, 7, 2, 4, 1), (0, 1, 2, 3, 4, 5, 6, 7)]}
SENTINEL = -7.25


@pytest.mark.gpu
@pytest.mark.parametrize('s', [1, 8, 33, 40, 64])
@pytest.mark.parametrize('k', [1, 2, 4, 8])
def test_reduce_equals_its_torch_restatement_bit_for_bit(pkg, dev, k, s):
    ops = pkg.ops
    g = torch.Generator().manual_seed(1000 * k + s)
    for b in (1, 3):
        for c in (1, 2, 3):
            stack = ops.new_tta_stack(k, b, c, s, dev)
            assert tuple(stack.shape) == (k, b, c, s, s)
            stack.copy_(torch.rand(k, b, c, s, s, generator=g))
            for v in range(k):
                assert ops.nhwc_ld(stack[v]) == 4
                _raw(stack[v])[..., c:] = float('nan')                           # every pad lane of the input
            assert not torch.isnan(stack).any()
            for codes in CODE_LISTS[k]:
                want = R.tree_mean_t([R.T_inv_t(stack[v], code) for v, code in enumerate(codes)])
                big = ops.new_nhwc(b + 2, c, s, s, dev)
                _raw(big).fill_(SENTINEL)
                out = ops.sw_tta_reduce(stack, codes, out=big[1:1 + b])
                assert out.data_ptr() == big[1:1 + b].data_ptr()
                raw = _raw(big)
                assert torch.equal(big[1:1 + b], want), (b, c, codes)
                assert not raw[1:1 + b, ..., c:].view(torch.int32).any()         # pad lanes of the result: +0.0, no NaN came along
                assert bool((raw[0] == SENTINEL).all()) and bool((raw[1 + b] == SENTINEL).all())
            # a fresh result, and a list of views instead of the stack
            fresh = ops.sw_tta_reduce([stack[v] for v in range(k)], CODE_LISTS[k][0])
            assert torch.equal(fresh, R.tree_mean_t([R.T_inv_t(stack[v], code) for v, code in enumerate(CODE_LISTS[k][0])]))
            assert ops.nhwc_ld(fresh) == 4 and not _raw(fresh)[..., c:].view(torch.int32).any()


@pytest.mark.gpu
def test_reduce_of_a_batch_slice_of_a_larger_stack(pkg, dev):
    """`segment_image`'s last, partial batch: the first 2 samples of every view of a stack allocated for 5."""
    ops = pkg.ops
    stack = ops.new_tta_stack(4, 5, 3, 33, dev)
    stack.copy_(torch.rand(4, 5, 3, 33, 33, generator=torch.Generator().manual_seed(5)))
    codes = (1, 6, 0, 7)
    got = ops.sw_tta_reduce(stack[:, :2], codes)
    assert torch.equal(got, R.tree_mean_t([R.T_inv_t(stack[v, :2], code) for v, code in enumerate(codes)]))


@pytest.mark.gpu
def test_reduce_of_equal_views_of_a_symmetric_map_gives_the_map_back(pkg, dev):
    """K equal inputs give back exactly that input: a map invariant under all of D4, in all eight slabs."""
    ops = pkg.ops
    a = torch.rand(2, 3, 40, 40, generator=torch.Generator().manual_seed(6))
    sym = torch.stack([R.T_t(a, k) for k in range(8)]).amax(0)               # max is exact and order-free
    assert all(torch.equal(R.T_t(sym, k), sym) for k in range(8))
    stack = ops.new_tta_stack(8, 2, 3, 40, dev)
    stack.copy_(sym.expand(8, 2, 3, 40, 40))
    assert torch.equal(ops.sw_tta_reduce(stack, 'd4').cpu(), sym)


# ----------------------------------------------------------------------------- [11] identity on an equivariant model
class _Pointwise(torch.nn.Module):
    """One 1x1 convolution with bias: no pixel sees another, so the model commutes with every view."""

    def __init__(self, ops, seed):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.ops = ops
        self.weight = torch.nn.Parameter(torch.randn(3, 3, 1, 1, generator=g) * 150.0)
        self.bias = torch.nn.Parameter(torch.randn(3, generator=g) * 0.2)

    def forward(self, x):
        return self.ops.conv2d(x, self.weight, self.bias)


@pytest.mark.gpu
@pytest.mark.parametrize('h,w,p_size,size', [(70, 75, 32, 16), (70, 75, 32, 32)])
def test_tta_of_an_equivariant_model_changes_nothing(pkg, dev, h, w, p_size, size):
    A, ops = pkg.aerial_image_segmentation_api, pkg.ops
    model = _Pointwise(ops, 80).to(dev).eval()
    img = _image(h, w, 81)
    org = A.patch_origins(h, w, p_size, 0.5)[:5]
    with torch.no_grad():
        x = ops.sw_gather_patches(torch.from_numpy(img).to(dev), org, p_size, size)
        y = model(x)
        for k in range(8):
            if not torch.equal(model(ops.sw_gather_patches(torch.from_numpy(img).to(dev), org, p_size, size, orient=k)), R.T_t(y, k)):
                pytest.skip('the 1x1 conv route is not position-independent bit for bit (view %d): the identity cannot be tested on it' % k)
    cfg = _cfg(p_size, size)
    masks, probs, org0, wts0 = A.segment_image(model, img, cfg, batch_size=5, return_probs=True)
    assert all(set(np.unique(m)) == {0, 255} for m in masks), 'constant masks: the case tests nothing'
    for tta in SETS + ((3, 5),):
        m, p, o, wt = A.segment_image(model, img, cfg, batch_size=5, return_probs=True, tta=tta)
        assert (o, wt) == (org0, wts0)
        assert np.array_equal(p, probs), tta
        assert all(np.array_equal(a, b) for a, b in zip(m, masks)), tta


# ----------------------------------------------------------------------------- [12] composition on the real generator
@pytest.fixture(scope='module')
def model(pkg, dev):
    torch.manual_seed(41)
    m = pkg.archs.UNet_R_SS_v2(3, 3, False).to(dev)
    m.train()
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        m(torch.randn(2, 3, 64, 64, generator=g).to(dev))                    # non-trivial running statistics
    return m.eval()


def _written_out(pkg, model, img, cfg, batch_size, dedupe, codes, precision='fp32'):
    """The loop `tta` stands for, with orient = 0 gathers and torch views: (probabilities [P, C, S, S] on the device, origins, weights)."""
    A, ops = pkg.aerial_image_segmentation_api, pkg.ops
    p_size, size = cfg['patch_size'], cfg['input_w']
    org = A.patch_origins(img.shape[0], img.shape[1], p_size, cfg['patch_overlap'])
    org, wts = A.unique_origins(org) if dedupe else (org, [1] * len(org))
    dimg = torch.from_numpy(img).to(next(model.parameters()).device)
    outs = []
    with torch.no_grad(), ops.infer_precision(precision):
        for i in range(0, len(org), batch_size):
            x = ops.sw_gather_patches(dimg, org[i:i + batch_size], p_size, size)
            qs = [R.T_inv_t(ops.sigmoid(model(R.T_t(x, k))), k) for k in codes]
            outs.append(R.tree_mean_t(qs))
    return torch.cat(outs, 0), org, wts


@pytest.mark.gpu
@pytest.mark.parametrize('p_size,dedupe,batch_size,precision', [(64, True, 6, 'fp32'), (64, False, 12, 'fp32'), (128, True, 3, 'fp32'),
                                                                (128, False, 3, 'fp32'), (128, True, 3, 'bf16x1')])
def test_d4_on_the_generator_equals_the_loop_written_out(pkg, dev, model, p_size, dedupe, batch_size, precision):
    A, ops = pkg.aerial_image_segmentation_api, pkg.ops
    h, w, size = 192, 160, 64
    cfg, img = _cfg(p_size, size), _image(h, w, 90)
    codes = ops.tta_codes('d4')
    want, org, wts = _written_out(pkg, model, img, cfg, batch_size, dedupe, codes, precision)
    assert len(org) % batch_size != 0                                           # a partial last batch
    masks, probs, got_org, got_wts = A.segment_image(model, img, cfg, batch_size=batch_size, dedupe=dedupe, return_probs=True,
                                                     precision=precision, tta='d4')
    assert (got_org, got_wts) == (org, wts)
    assert probs.shape == (len(org), 3, size, size) and np.array_equal(probs, want.cpu().numpy())
    want_masks = ops.sw_merge_masks(want, org, wts, p_size, h, w).cpu().numpy()
    assert all(np.array_equal(masks[c], want_masks[c]) for c in range(3))
    plain = A.segment_image(model, img, cfg, batch_size=batch_size, dedupe=dedupe, return_probs=True, precision=precision)[1]
    assert not np.array_equal(plain, probs)                                     # the generator is not equivariant: TTA did something


# ----------------------------------------------------------------------------- [13] evaluation
@pytest.mark.gpu
def test_evaluate_image_counts_the_tta_masks(pkg, dev, model):
    A, ops = pkg.aerial_image_segmentation_api, pkg.ops
    h, w, p_size, size = 192, 160, 128, 64
    cfg, img, lab = _cfg(p_size, size), _image(h, w, 91), label_image(192, 160, 3, 92)
    masks, gt = A.segment_image(model, img, cfg, batch_size=4, label_bgr=lab, tta='flips')
    _, gt_plain = A.segment_image(model, img, cfg, batch_size=4, label_bgr=lab)
    assert all(np.array_equal(a, b) for a, b in zip(gt, gt_plain))
    want = ops.sw_mask_counts(torch.from_numpy(np.stack(masks)).to(dev), torch.from_numpy(np.stack(gt)).to(dev))
    got = A.evaluate_image(model, img, lab, cfg, batch_size=4, tta='flips')
    assert got.dtype == torch.int64 and torch.equal(got, want) and int(want[:, 2].min()) > 0
    res = A.evaluate_images(model, [(img, lab), (img, lab)], cfg, batch_size=4, tta='flips')
    assert np.array_equal(res['counts'], 2 * want.cpu().numpy())


# ----------------------------------------------------------------------------- [14] the default is untouched
@pytest.mark.gpu
@pytest.mark.parametrize('dedupe', [True, False])
def test_default_and_the_identity_view_are_todays_pipeline(pkg, dev, model, dedupe):
    A, ops = pkg.aerial_image_segmentation_api, pkg.ops
    h, w, p_size, size, bs = 192, 160, 128, 64, 3
    cfg, img = _cfg(p_size, size), _image(h, w, 93)
    org = A.patch_origins(h, w, p_size, 0.5)
    org, wts = A.unique_origins(org) if dedupe else (org, [1] * len(org))
    dimg = torch.from_numpy(img).to(dev)
    probs = ops.new_nhwc(len(org), 3, size, size, dev)
    with torch.no_grad():                                                       # the statements of the pipeline before `tta`
        for i in range(0, len(org), bs):
            ops.sigmoid_into(model(ops.sw_gather_patches(dimg, org[i:i + bs], p_size, size)), probs[i:i + bs])
        want_masks = ops.sw_merge_masks(probs, org, wts, p_size, h, w).cpu().numpy()
    want_probs = probs.cpu().contiguous().numpy()
    for tta in (None, (0,)):
        masks, got, o, wt = A.segment_image(model, img, cfg, batch_size=bs, dedupe=dedupe, return_probs=True, tta=tta)
        assert (o, wt) == (org, wts)
        assert np.array_equal(got, want_probs), tta
        assert all(np.array_equal(masks[c], want_masks[c]) for c in range(3)), tta
