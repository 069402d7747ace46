"""Sliding-window full-image inference, MI355X-native (mirrors the GPU side of the reference's
scripts/aerial_image_segmentation_api.py -- SURVEY.md 8f row N2 / BASELINE config 5).

GPU side: the eval-mode generator forward over all patches of an image.  The reference runs one patch per forward
(`api.py:385-390`); here patches are batched and every BasicBlock runs as three MFMA launches with its batch norms folded
in, then one sigmoid kernel -- same values, no per-patch sync.  `segment_image` also runs the two host loops around the
forwards (patch cutting / resizing / normalisation, and `patch_merge`) as HIP kernels, bit for bit what the host functions
below compute; those stay as the oracle.  With a label image it runs the ground-truth branch (`mask_convert` per patch and class,
a second `patch_merge`, `api.py:220-236,394-406`) on the device too, and `evaluate_image` / `evaluate_images` reduce the two mask
sets to per-class pixel counts (IoU, Dice) there, without downloading a mask.  Not in the reference, which cuts at 127 only: the
per-pixel confidence maps behind `patch_merge` (`patch_merge_scores`, `segment_image(..., threshold=, return_scores=)`) and the sweep
of IoU / Dice over all 255 levels from one histogram (`evaluate_images(..., sweep=True)`).  The overlay JPGs (`save_masking*`), PNG decoding,
non-square inference sizes and resize factors other than 1 and 2 are not covered.

Host side (numpy, no cv2 / albumentations -- neither is installed here, and the package takes on no host dependency for
them): `load_segmentation_models` (`api.py:302-333`), `get_patched_input` (`api.py:336-373`, including its double
normalisation: albumentations `Normalize()` and THEN `/ 255` again, `:354-367`), the patch order of `patch_gen`
(`api.py:45-116`), `patch_merge` with its uint8 round trip, 2x resize and threshold post-processing (`api.py:33-42,119-217`)
and `mask_convert` (`api.py:218-234`).  What replaces the two library calls, and how it is pinned:
  * `cv2.resize` (default INTER_LINEAR) is restated for the two exact factors the pipeline uses -- 1/2 (1024 -> 512: the
    half-pixel-centre bilinear kernel is exactly the 2x2 box mean) and 2 (512 -> 1024: 0.25 / 0.75 taps, edge-clamped),
    rounded half up like OpenCV's fixed-point path; any other factor raises.  cv2 is absent from this environment, so
    this restatement is NOT pinned by a reference-generated vector (OpenCV's two-pass fixed-point rounding can differ by
    one grey level); downstream of `patch_merge` every resized value is thresholded at 127, so a one-level difference
    matters only for interpolated values of exactly 127 or 128.
  * albumentations `Normalize()` defaults (mean (0.485, 0.456, 0.406), std (0.229, 0.224, 0.225), max_pixel_value 255) in
    its float32 arithmetic order; applied, as the reference does, to the BGR channel order `cv2.imread` yields.
"""
import json
import math
import os

import numpy as np
import torch

from . import archs, ops


def patch_origins(img_h, img_w, p_size, overlap=0.5):
    """(h1, w1) of every patch in the reference's order: four sweeps anchored at the top-left,
    bottom-right, bottom-left and top-right corners (api.py:45-116)."""
    step = int(math.ceil((1 - overlap) * p_size))
    i_w = int(math.floor((img_w - p_size) / step)) + 1
    i_h = int(math.floor((img_h - p_size) / step)) + 1
    sweeps = []
    for anchor_bottom, anchor_right in ((False, False), (True, True), (True, False), (False, True)):
        for i in range(i_w):
            for j in range(i_h):
                w1 = img_w - i * step - p_size if anchor_right else i * step
                h1 = img_h - j * step - p_size if anchor_bottom else j * step
                if h1 < 0 or w1 < 0 or h1 + p_size > img_h or w1 + p_size > img_w:
                    raise ValueError('patch outside the image (img %dx%d, patch %d)' % (img_h, img_w, p_size))
                sweeps.append((h1, w1))
    return sweeps


def patch_gen(img, mask, p_size, overlap=0.5):
    org = patch_origins(img.shape[0], img.shape[1], p_size, overlap)
    return ([img[h:h + p_size, w:w + p_size, :] for h, w in org], [mask[h:h + p_size, w:w + p_size, :] for h, w in org])


_GRAPHS = {}


def _cached_operands(model):
    """Every tensor the packed-weight (`ops._pack`, `ops._x1_pack`, `bf16._pack`), BN-fold (`BasicBlock._folded`) and gamma|beta-concat
    (`blocks._spade_cat`) caches of `model` hold right now."""
    held = []
    for t in list(model.parameters()) + list(model.buffers()):
        for name in ('_ssg_pack', '_ssg_pack_bf16', '_ssg_pack_bf16x1', '_ssg_pack_bf16x2'):
            c = t.__dict__.get(name)
            if c is not None:
                held += list(c[1].values())
        c = t.__dict__.get('_ssg_gb_cat')
        if c is not None:
            held += [c[1], c[2]]
    for m in model.modules():
        c = getattr(m, '_fold_cache', None)
        if c is not None:
            held += list(c[1])
            for t in c[1]:                       # the folded weights are themselves packed per use
                for name in ('_ssg_pack', '_ssg_pack_bf16x1', '_ssg_pack_bf16x2'):
                    p = t.__dict__.get(name)
                    if p is not None:
                        held += list(p[1].values())
    return held


def _graph_for(model, shape, device, precision='fp32'):
    """hipGraph of `sigmoid(model(x))` for one input shape (eval mode), captured after a warm-up call that fills the
    packed-weight and BN-fold caches; tied to the parameter values it was captured with (keyed by the weight / statistics
    epochs) and to the `precision` it was captured under (`ops.infer_precision`: an fp32 capture is never replayed for a
    bf16x1 request, nor the other way round).  MEASURED (profiles/r02_a_bench_extra.jsonl): one 3x512x512 patch takes 6.52 ms launched kernel by kernel and
    6.48 ms as a graph replay -- the ~330 launches of a batch-1 forward are NOT what limits the patch rate (round 1 assumed
    so); the deep levels do (16x16 x 768 channels at batch 1 is 12 workgroups of 432 K-steps on a 256-CU chip).  The graph
    path is therefore opt-in (`graph=True`), kept because it takes the Python launch path off the host for callers that
    overlap other host work."""
    # The capture bakes in the ADDRESSES of the packed-weight / BN-fold tensors the warm-up call cached, so it is valid for
    # exactly one state of every parameter and buffer: (storage address, autograd version) of each -- what the caches themselves
    # stamp with -- plus the two epochs that cover raw-pointer writes.  load_state_dict() / any in-place edit changes a version
    # and forces a new capture instead of replaying the old weights.
    stamp = tuple((t.data_ptr(), t._version) for t in list(model.parameters()) + list(model.buffers()))
    key = (id(model), tuple(shape), str(device), ops._WEIGHT_EPOCH[0], ops._STATS_EPOCH[0], hash(stamp), precision)
    hit = _GRAPHS.get(key)
    if hit is not None and hit[0]() is model and hit[4] == stamp:
        return hit[1:4]
    import weakref
    static_in = torch.zeros(shape, dtype=torch.float32, device=device)
    side = torch.cuda.Stream(device=device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side), ops.infer_precision(precision):   # warm-up on the capture stream: caches, lazy kernel attributes
        ops.sigmoid(model(static_in))
    torch.cuda.current_stream(device).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with ops.infer_precision(precision), torch.cuda.graph(graph):
        static_out = ops.sigmoid(model(static_in))
    for k in [k for k, v in _GRAPHS.items() if v[0]() is None or (k[0] == id(model) and k[1] == tuple(shape) and k[-1] == precision)]:
        del _GRAPHS[k]                                  # stale captures of this model / dead models
    # keep what the captured kernels read alive for as long as the capture: a later eager forward with other weights
    # re-fills the caches and would otherwise free these tensors under the graph
    _GRAPHS[key] = (weakref.ref(model), graph, static_in, static_out, stamp, _cached_operands(model))
    return graph, static_in, static_out


def infer_patches(model, img_patch_set, batch_size=16, graph=False, precision='fp32'):
    """sigmoid(model(patch)) for every patch, batched.  img_patch_set: [P, C, H, W] float32 (numpy or
    tensor, as `get_patched_input` builds it); returns a float32 tensor [P, num_classes, H, W] on the host.
    `graph=True`: replay a captured hipGraph per batch instead of launching kernel by kernel (same values; see _graph_for).
    `precision`: 'fp32' (default: today's kernels, bit for bit) or 'bf16x1' -- an APPROXIMATION that trades the fp32 guarantee for
    speed: the 3x3 stride-1 convs of the model's eval-mode BasicBlocks whose shape the one-term kernel takes (32-channel multiples
    in, 64 out, at least 17 pixels wide: not the stem's 3-channel conv, not the 16x16 levels) round x and the BN-folded weights
    once to bf16 and accumulate in fp32 (`ops.conv2d_bf16x1`).  The 1x1 shortcuts, stride-2 convs, SPADE, pooling and resampling
    layers and every tensor in memory stay fp32.  'bf16x2': the same convs with each operand split into two bf16 terms and three
    products kept (`ops.conv2d(..., precision='bf16x2')`): |error| <= (3 * 2^-16 + 3 * 2^-32) conv(|x|, |w|) per conv, half the matrix
    instructions of the default.  Any other string raises ValueError."""
    x = torch.as_tensor(img_patch_set, dtype=torch.float32)
    model.eval()
    outs = []
    with torch.no_grad(), ops.infer_precision(precision):
        for i in range(0, x.shape[0], batch_size):
            xb = x[i:i + batch_size].cuda(non_blocking=True)
            if graph:
                g, static_in, static_out = _graph_for(model, xb.shape, xb.device, precision)
                static_in.copy_(xb)
                g.replay()
                y = static_out.clone()
            else:
                y = ops.sigmoid(model(xb))
            outs.append(y)
    out = torch.cat([o.contiguous() for o in outs], 0) if len(outs) > 1 else outs[0].contiguous()
    return out.cpu()


def patch_merge_mean(img_h, img_w, masks, p_size, p_overlap, num_classes):
    """Overlap-average of per-patch probability maps at patch resolution (the arithmetic core of
    patch_merge, api.py:119-217, without the uint8 round trip, cv2.resize and hysteresis)."""
    org = patch_origins(img_h, img_w, p_size, p_overlap)
    if len(org) != len(masks):
        raise ValueError('expected %d patches, got %d' % (len(org), len(masks)))
    merged = np.zeros((num_classes, img_h, img_w), dtype=np.float64)
    div = np.zeros((img_h, img_w), dtype=np.float64)
    for (h, w), m in zip(org, masks):
        m = np.asarray(m)
        if m.shape[-2:] != (p_size, p_size):
            raise NotImplementedError('inference size != patch size needs the cv2.resize step of the reference')
        merged[:, h:h + p_size, w:w + p_size] += m
        div[h:h + p_size, w:w + p_size] += 1
    div[div == 0] = 1.0
    return merged / div


def segmentation_inference(model, img_input, img_patch_set, mask_patch_set, config, gt_mask_flag=False, batch_size=16):
    """api.py:376-410 for the prediction branch: batched GPU inference + overlap averaging."""
    probs = infer_patches(model, img_patch_set, batch_size).numpy()
    all_class_mask = patch_merge_mean(img_input.shape[0], img_input.shape[1], list(probs), config['patch_size'],
                                      config['patch_overlap'], config['num_classes'])
    return all_class_mask, all_class_mask


# ----------------------------------------------------------------------------- host half (api.py:33-42,218-234,302-373)
def post_process_resized_mask(resized_mask):
    """api.py:33-42: values in (127, 255) -> 255, values in (0, 127] -> 0 (in place, like the reference)."""
    half_th = 127
    resized_mask[(resized_mask > half_th) & (resized_mask < 255)] = 255
    resized_mask[(resized_mask > 0) & (resized_mask <= half_th)] = 0
    return resized_mask


def resize_u8(img, out_h, out_w):
    """cv2.resize(img, (out_w, out_h)) (INTER_LINEAR) for uint8 images at the exact factors 1, 1/2 and 2 (module docstring)."""
    img = np.asarray(img)
    if img.dtype != np.uint8:
        raise TypeError('resize_u8 expects uint8')
    h, w = img.shape[:2]
    if (out_h, out_w) == (h, w):
        return img.copy()
    if h == 2 * out_h and w == 2 * out_w:                 # src = 2*dst + 0.5: mean of a 2x2 box
        a = img.astype(np.uint16)
        s4 = a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2]
        return ((s4 + 2) >> 2).astype(np.uint8)
    if out_h == 2 * h and out_w == 2 * w:                 # src = dst/2 - 0.25: taps (0.25, 0.75) / (0.75, 0.25), clamped at the edges
        def up(a, axis):
            a = np.moveaxis(a, axis, 0)
            prev = np.concatenate([a[:1], a[:-1]], 0); nxt = np.concatenate([a[1:], a[-1:]], 0)
            out = np.empty((2 * a.shape[0],) + a.shape[1:], dtype=np.float64)
            out[0::2] = 0.25 * prev + 0.75 * a
            out[1::2] = 0.75 * a + 0.25 * nxt
            return np.moveaxis(out, 0, axis)
        f = up(up(img.astype(np.float64), 0), 1)
        return np.floor(f + 0.5).astype(np.uint8)
    raise NotImplementedError('resize_u8: only the exact factors 1, 1/2 and 2 of the sliding-window pipeline are restated '
                              '(%dx%d -> %dx%d needs cv2.resize)' % (h, w, out_h, out_w))


def normalize_imagenet(img):
    """albumentations.Normalize() with its defaults on an HxWx3 uint8 image, float32 arithmetic in its order."""
    mean = np.array((0.485, 0.456, 0.406), dtype=np.float32) * 255.0
    std = np.array((0.229, 0.224, 0.225), dtype=np.float32) * 255.0
    denom = np.reciprocal(std, dtype=np.float32)
    out = img.astype(np.float32)
    out -= mean
    out *= denom
    return out


def imread_bgr(path):
    """cv2.imread(path): HxWx3 uint8 in BGR order (decoded with PIL)."""
    from PIL import Image
    with Image.open(path) as im:
        rgb = np.asarray(im.convert('RGB'))
    return np.ascontiguousarray(rgb[:, :, ::-1])


def get_patched_input(img_path, config, gt_mask_flag, imread=imread_bgr):
    """api.py:336-373.  Returns (img_input, img_patch_set [P, 3, input_w, input_w] float32, mask_patch_set)."""
    p_size, img_size, patch_overlap = config['patch_size'], config['input_w'], config['patch_overlap']
    img_input = imread(img_path)
    mask_input = imread(img_path.replace('image', 'labels')) if gt_mask_flag is True else img_input
    image_patch, mask_patch = patch_gen(img_input, mask_input, p_size, patch_overlap)
    if (config['input_h'], config['input_w']) != (img_size, img_size):
        raise NotImplementedError('non-square inference size')
    img_patch_set = []
    for img in image_patch:
        img = resize_u8(img, img_size, img_size)                     # :359; the Resize() of the transform is then the identity
        img = normalize_imagenet(img)                                # :364-365 (transforms.Normalize())
        img = img.astype('float32') / 255                            # :367 -- yes, a second division by 255
        img_patch_set.append(img.transpose(2, 0, 1))
    return img_input, np.array(img_patch_set), np.array(mask_patch)


def mask_convert(p_mask, idx, p_size):
    """api.py:218-234: class idx of a BGR label patch -> {0, 255} mask at p_size."""
    want = {0: (255, 255, 255), 1: (255, 0, 0), 2: (0, 0, 255)}[idx]
    sel = (p_mask[:, :, 0] == want[0]) & (p_mask[:, :, 1] == want[1]) & (p_mask[:, :, 2] == want[2])
    mask = (sel.astype(np.float64) * 255).astype('uint8')
    return post_process_resized_mask(resize_u8(mask, p_size, p_size))


def patch_merge(img, masks, p_size, config, p_overlap):
    """api.py:119-217: per class, every patch's probability map -> uint8 -> resized to p_size -> thresholded -> overlap
    average -> uint8 -> thresholded again.  Returns a list of num_classes uint8 [H, W] masks with values {0, 255}."""
    img_h, img_w = img.shape[0], img.shape[1]
    org = patch_origins(img_h, img_w, p_size, p_overlap)
    if len(org) != len(masks):
        raise ValueError('expected %d patches, got %d' % (len(org), len(masks)))
    all_class_mask = []
    for c in range(config['num_classes']):
        merged = np.zeros((img_h, img_w)); div = np.zeros((img_h, img_w))
        for (h1, w1), m in zip(org, masks):
            mask = (np.asarray(m[c]) * 255).astype('uint8')
            resized = post_process_resized_mask(resize_u8(mask, p_size, p_size)) / 255.0
            merged[h1:h1 + p_size, w1:w1 + p_size] += resized
            div[h1:h1 + p_size, w1:w1 + p_size] += 1.0
        div[div == 0] = 1.0
        full = (np.divide(merged, div) * 255).astype('uint8')
        all_class_mask.append(post_process_resized_mask(full))
    return all_class_mask


def patch_merge_scores(img, masks, p_size, config, p_overlap):
    """The confidence map behind `patch_merge`: per class a uint8 [H, W] score S in 0 .. 255, the number of
    first-stage levels t in 0 .. 254 at which `patch_merge`, with `resized > t` in place of its `resized > 127` per patch and its
    second stage unchanged, turns the pixel on.  Raising t only removes votes, so `S > t` IS that merge and `S > 127` is
    `patch_merge` itself.  Plain numpy, the 255 merges written out: the per-patch resize is done once, the votes are summed in
    fp64 (0.0 / 1.0 terms, exact in any order) for a block of levels at a time, and each level goes through `patch_merge`'s own
    `(merged / div * 255).astype('uint8') > 127`.  Returns a list of num_classes arrays."""
    img_h, img_w = img.shape[0], img.shape[1]
    org = patch_origins(img_h, img_w, p_size, p_overlap)
    if len(org) != len(masks):
        raise ValueError('expected %d patches, got %d' % (len(org), len(masks)))
    div = np.zeros((img_h, img_w))
    for h1, w1 in org:
        div[h1:h1 + p_size, w1:w1 + p_size] += 1.0
    div[div == 0] = 1.0
    block = max(1, min(255, (1 << 23) // (img_h * img_w)))             # levels merged at once: at most 64 MiB of fp64 votes
    all_class_score = []
    for c in range(config['num_classes']):
        resized = [resize_u8((np.asarray(m[c]) * 255).astype('uint8'), p_size, p_size) for m in masks]
        score = np.zeros((img_h, img_w), dtype=np.int64)
        for t0 in range(0, 255, block):
            levels = np.arange(t0, min(t0 + block, 255)).reshape(-1, 1, 1)
            merged = np.zeros((levels.shape[0], img_h, img_w))
            for (h1, w1), r in zip(org, resized):
                merged[:, h1:h1 + p_size, w1:w1 + p_size] += (r[None] > levels)
            full = (np.divide(merged, div) * 255).astype('uint8')
            score += (full > 127).sum(0)
        all_class_score.append(score.astype(np.uint8))
    return all_class_score


def score_hist(scores, gt):
    """int64 [C, 2, 256]: per class c and g = (gt[c] > 127), how many pixels have each score -- the host form of
    `ops.sw_score_hist`.  `scores`, `gt`: [C, H, W] uint8 arrays or lists of C [H, W] arrays."""
    scores, gt = np.asarray(scores), np.asarray(gt)
    if scores.dtype != np.uint8 or gt.dtype != np.uint8 or scores.shape != gt.shape:
        raise TypeError('score_hist expects two uint8 arrays of one shape')
    return np.stack([np.bincount(s.ravel().astype(np.int64) + 256 * (g.ravel() > 127), minlength=512).reshape(2, 256)
                     for s, g in zip(scores, gt)]).astype(np.int64)


def threshold_curves(hist):
    """IoU and Dice of every first-stage level from a score histogram int64 [C, 2, 256] (`score_hist`, `ops.sw_score_hist`): with
    I(t) = sum over s > t of hist[c, 1, s], P(t) = sum over s > t of hist[c, 0, s] + hist[c, 1, s] and G = sum of hist[c, 1, :],
    `iou_curve`[c, t] = (I + 1e-5) / (P + G - I + 1e-5) and `dice_curve`[c, t] = (2 I + 1e-5) / (P + G + 1e-5) for t in 0 .. 254
    (float64 [C, 255], the smoothing of `evaluate_images`); `best_threshold`[c] the level of the largest IoU, the lowest one on
    ties, and `best_iou`[c] that IoU."""
    hist = np.asarray(hist)
    if hist.ndim != 3 or hist.shape[1:] != (2, 256):
        raise ValueError('threshold_curves expects a [C, 2, 256] histogram, got %s' % (hist.shape,))
    hist = hist.astype(np.int64)
    above = np.cumsum(hist[:, :, ::-1], axis=2)[:, :, ::-1][:, :, 1:]   # [C, 2, 255]: pixels with score > t
    i, p = above[:, 1], above[:, 0] + above[:, 1]
    g = hist[:, 1].sum(1, keepdims=True)
    smooth = 1e-5
    iou = (i + smooth) / (p + g - i + smooth)
    dice = (2 * i + smooth) / (p + g + smooth)
    best = iou.argmax(1)                                                # first maximum: the lowest level on ties
    return dict(iou_curve=iou, dice_curve=dice, best_threshold=[int(b) for b in best],
                best_iou=[float(iou[c, b]) for c, b in enumerate(best)])


# ----------------------------------------------------------------------------- the whole pipeline on the device
def unique_origins(org):
    """(distinct origins of `org` in order of first appearance, how often each occurs).  The four corner-anchored sweeps of
    `patch_origins` coincide whenever (image - patch) is a multiple of the step: at the shipped geometry (2048^2, patch 1024,
    overlap 0.5) the 36 patches have 9 distinct origins, each four times."""
    count = {}
    for o in org:
        o = (int(o[0]), int(o[1]))
        count[o] = count.get(o, 0) + 1                   # dicts keep insertion order
    return list(count.keys()), list(count.values())


def _device_masks(model, img_bgr, config, batch_size, dedupe, precision, label_bgr, who, tta=None, threshold=None,
                  want_scores=False, want_masks=True):
    """The device half of `segment_image` / `evaluate_image`: (prediction masks [C, H, W] uint8 on the device, ground-truth masks
    likewise or None, probabilities, origins, weights, score maps [C, H, W] uint8 or None).  `threshold`: the masks at these
    first-stage levels (`ops.sw_merge_scores` in mask mode) instead of `ops.sw_merge_masks`; `want_scores`: the score maps too;
    `want_masks=False`: no prediction masks (None).  Every check runs before the first upload or launch."""
    codes = None if tta is None else ops.tta_codes(tta)
    p_size, size, overlap, classes = config['patch_size'], config['input_w'], config['patch_overlap'], config['num_classes']
    levels = None
    if threshold is not None:
        levels = ops.sw_levels(threshold, classes, who)
        if classes > 64:
            raise ValueError('%s: thresholds for %d classes: at most 64 classes take levels' % (who, classes))
    if (config['input_h'], config['input_w']) != (size, size):
        raise NotImplementedError('non-square inference size')
    img_bgr = np.asarray(img_bgr)
    if img_bgr.dtype != np.uint8 or img_bgr.ndim != 3 or img_bgr.shape[2] != 3:
        raise TypeError('%s expects an HxWx3 uint8 image' % who)
    if label_bgr is not None:
        label_bgr = np.asarray(label_bgr)
        if label_bgr.dtype != np.uint8:
            raise TypeError('%s expects a uint8 label image' % who)
        if label_bgr.shape != img_bgr.shape:
            raise ValueError('%s: the label image is %s, the image %s' % (who, label_bgr.shape, img_bgr.shape))
        if not 1 <= classes <= 3:
            raise ValueError('%s: %d classes: the label palette (mask_convert) has 3 colours' % (who, classes))
    img_h, img_w = img_bgr.shape[0], img_bgr.shape[1]
    org = patch_origins(img_h, img_w, p_size, overlap)
    org, weights = unique_origins(org) if dedupe else (org, [1] * len(org))
    dev = next(model.parameters()).device
    img = torch.from_numpy(np.ascontiguousarray(img_bgr)).to(dev)
    probs = ops.new_nhwc(len(org), classes, size, size, dev)
    model.eval()
    gt_masks = None
    with torch.no_grad(), ops.infer_precision(precision):
        if codes is None:
            for i in range(0, len(org), batch_size):
                x = ops.sw_gather_patches(img, org[i:i + batch_size], p_size, size)
                ops.sigmoid_into(model(x), probs[i:i + batch_size])
        else:                                            # every view of a batch, then their mean mapped back
            stack = ops.new_tta_stack(len(codes), min(batch_size, len(org)), classes, size, dev)
            for i in range(0, len(org), batch_size):
                n = len(org[i:i + batch_size])
                for v, k in enumerate(codes):
                    x = ops.sw_gather_patches(img, org[i:i + batch_size], p_size, size, orient=k)
                    ops.sigmoid_into(model(x), stack[v, :n])
                ops.sw_tta_reduce(stack[:, :n], codes, out=probs[i:i + batch_size])
        masks = scores = None
        if want_masks and levels is None:
            masks = ops.sw_merge_masks(probs, org, weights, p_size, img_h, img_w)
        elif want_masks:
            masks = ops.sw_merge_scores(probs, org, weights, p_size, img_h, img_w, thresholds=levels)
        if want_scores:
            scores = ops.sw_merge_scores(probs, org, weights, p_size, img_h, img_w)
        if label_bgr is not None:                        # api.py:394-406: mask_convert per patch and class, then patch_merge
            label = torch.from_numpy(np.ascontiguousarray(label_bgr)).to(dev)
            gt = ops.sw_gather_labels(label, org, p_size, size, classes)
            gt_masks = ops.sw_merge_masks(gt, org, weights, p_size, img_h, img_w)
    return masks, gt_masks, probs, org, weights, scores


def segment_image(model, img_bgr, config, batch_size=12, dedupe=True, return_probs=False, precision='fp32', label_bgr=None, tta=None,
                  threshold=None, return_scores=False):
    """`segmentation_inference_full(model, *get_patched_input(...), config, False)[0]` for an image already in memory, with
    everything between the uint8 image and the uint8 masks on the device: the image is uploaded once, each batch of patches is
    cut, resized and normalised by `ops.sw_gather_patches`, `sigmoid(model(x))` stays on the device, `ops.sw_merge_masks` does
    `patch_merge`, and num_classes * H * W bytes come back.  Returns a list of num_classes uint8 [H, W] masks in {0, 255}.
    `dedupe`: infer each distinct origin once and let it enter the merge with its multiplicity (the same masks whenever
    equal patches give equal probabilities, which they do inside one batch composition).
    `return_probs`: also return (the host copy [P, C, S, S] of the probabilities that were merged, their origins, their weights).
    `precision`: 'fp32' (default, unchanged) or 'bf16x1', the approximation described at `infer_patches` (bf16 operand rounding in
    the BasicBlock 3x3 stride-1 convs); masks can differ from the fp32 path where a probability is near the threshold.
    `label_bgr`: the BGR label image of `img_bgr` (same shape, uint8) -- the ground-truth branch (`gt_mask_flag=True`, api.py:394-406)
    on the device: the label is uploaded once, `ops.sw_gather_labels` does `mask_convert` for every patch and class at the same
    origins, the same `ops.sw_merge_masks` merges them with the same weights, and the result becomes (masks, gt_masks) -- both
    lists of `segmentation_inference_full(..., gt_mask_flag=True)`, followed by the three `return_probs` items if asked for.  The
    ground-truth masks are integer arithmetic on the label alone: they depend on neither `dedupe` nor `precision`.  A label of
    another shape raises ValueError; num_classes above 3 raises ValueError (`mask_convert` has no colour for them).
    `tta`: flip / rotation test-time augmentation, not in the reference: None (default: the statements above, nothing added),
    'hflip', 'flips', 'd4' or a tuple of 1, 2, 4 or 8 distinct D4 codes (`ops.tta_codes`).  Each batch of patches is then gathered
    once per code k as T_k of the patch (`ops.sw_gather_patches(..., orient=k)`), inferred, and the K probability maps are mapped
    back by T_k^-1 and averaged by `ops.sw_tta_reduce` (balanced tree in list order, fp32) into the probabilities that are merged;
    K forwards per patch.  It composes with `dedupe`, `precision`, `label_bgr` and `return_probs`; the ground-truth masks do not
    depend on it.  Exact plumbing is what is tested; what it does to accuracy on a trained model is not measured here.  Anything
    else raises ValueError before the first upload or launch.
    `threshold`: the operating point, not in the reference, which hard-wires 127: None (default: the statements above, nothing
    added), an int in 0 .. 254 or a sequence of num_classes such ints.  The prediction masks are then `patch_merge` with every
    patch thresholded at that level instead of 127 (`ops.sw_merge_scores` in mask mode; 127 gives the default
    masks bit for bit); the second-stage level stays 127.  Bools and anything else raise ValueError before the first upload.
    `return_scores`: also return the confidence maps, a list of num_classes uint8 [H, W] arrays of scores S in 0 .. 255
    (`patch_merge_scores` is the host oracle): the mask at any level t is `S > t`.  They come last in the returned tuple, after the
    `return_probs` items.  Both compose with `dedupe`, `precision`, `tta`, `label_bgr` and `return_probs`; the ground-truth masks
    depend on neither.  Which level is best on a trained model is not measured here: there is no checkpoint.
    Not covered, as on the host path they stay with: the overlay JPGs, PNG decoding, non-square inference sizes and resize
    factors other than 1 and 2.  `evaluate_image` / `evaluate_images` turn the two mask sets into counts without a download."""
    classes = config['num_classes']
    masks, gt_masks, probs, org, weights, scores = _device_masks(model, img_bgr, config, batch_size, dedupe, precision, label_bgr,
                                                                 'segment_image', tta, threshold, bool(return_scores))
    masks = masks.cpu().numpy()
    masks = [masks[c] for c in range(classes)]
    out = (masks,)
    if label_bgr is not None:
        gt_masks = gt_masks.cpu().numpy()
        out += ([gt_masks[c] for c in range(classes)],)
    if return_probs:
        out += (probs.cpu().contiguous().numpy(), org, weights)
    if return_scores:
        scores = scores.cpu().numpy()
        out += ([scores[c] for c in range(classes)],)
    return out if len(out) > 1 else masks


def _hist_arg(hist, classes):
    """`hist` of `evaluate_image`, checked before any upload: None, True, or an int64 [classes, 2, 256] device tensor."""
    if hist is None or hist is True:
        return hist
    if not (isinstance(hist, torch.Tensor) and hist.is_cuda and hist.dtype == torch.int64 and tuple(hist.shape) == (classes, 2, 256)
            and hist.is_contiguous()):
        raise TypeError('evaluate_image: hist must be None, True or a contiguous int64 [%d, 2, 256] device tensor' % classes)
    return hist


def evaluate_image(model, img_bgr, label_bgr, config, batch_size=12, dedupe=True, precision='fp32', counts=None, tta=None, hist=None):
    """`segment_image(..., label_bgr=label_bgr)` with both mask sets kept on the device and reduced there by
    `ops.sw_mask_counts`: returns an int64 [num_classes, 3] DEVICE tensor of pixel counts per class -- (prediction and ground
    truth, prediction, ground truth) -- added into `counts` if such a tensor is given.  No mask is downloaded and nothing
    synchronises; read the tensor (`.cpu()`) when the numbers are needed.  `tta`: as in `segment_image`.
    `hist`: None (default: the statements above), True, or an int64 [num_classes, 2, 256] device tensor: the score maps
    (`ops.sw_merge_scores`) take the place of the prediction masks, and the return value is the histogram of their
    bytes per class and ground-truth bit (`ops.sw_score_hist`), added into that tensor if one is given -- every threshold's counts
    in one pass (`threshold_curves`).  A `counts` tensor given alongside still receives the level-127 counts (score > 127 is the
    mask).  Still no download and no synchronisation."""
    if tta is not None:
        ops.tta_codes(tta)
    if label_bgr is None:
        raise TypeError('evaluate_image needs a label image')
    if hist is None:
        masks, gt_masks, _, _, _, _ = _device_masks(model, img_bgr, config, batch_size, dedupe, precision, label_bgr, 'evaluate_image', tta)
        return ops.sw_mask_counts(masks, gt_masks, out=counts)
    hist = _hist_arg(hist, config['num_classes'])
    _, gt_masks, _, _, _, scores = _device_masks(model, img_bgr, config, batch_size, dedupe, precision, label_bgr, 'evaluate_image', tta,
                                                 want_scores=True, want_masks=False)
    if counts is not None:
        ops.sw_mask_counts(scores, gt_masks, out=counts)               # bit 7 of a score byte is the level-127 mask
    return ops.sw_score_hist(scores, gt_masks, out=None if hist is True else hist)


def evaluate_images(model, pairs, config, batch_size=12, dedupe=True, precision='fp32', tta=None, sweep=False):
    """`evaluate_image` over `pairs`, an iterable of (image, label), each an HxWx3 uint8 BGR array or a path read with
    `imread_bgr`; the counts accumulate on the device and are read once at the end.  Returns a dict: `counts`, a numpy int64
    [num_classes, 3] of (intersection I, prediction P, ground truth G) pixels per class over all images, and per class the
    Python floats `iou` = (I + 1e-5) / (P + G - I + 1e-5) and `dice` = (2 I + 1e-5) / (P + G + 1e-5) -- the smoothing of
    `metrics.iou_score`.  `tta`: as in `segment_image`.
    `sweep=True`: the threshold sweep -- the score histogram (`evaluate_image(..., hist=)`) accumulates over the images beside the
    counts and is read once; the dict then also carries `hist` (numpy int64 [num_classes, 2, 256]) and the items of
    `threshold_curves(hist)`: `iou_curve`, `dice_curve` ([num_classes, 255], one column per first-stage level 0 .. 254),
    `best_threshold` and `best_iou` per class.  `counts`, `iou` and `dice` stay the level-127 numbers of `sweep=False`.  What the
    best level does for a trained model is not measured here: there is no checkpoint."""
    if tta is not None:
        ops.tta_codes(tta)
    counts = hist = None
    for image, label in pairs:
        image = imread_bgr(image) if isinstance(image, (str, os.PathLike)) else image
        label = imread_bgr(label) if isinstance(label, (str, os.PathLike)) else label
        if sweep:
            if counts is None:
                counts = torch.zeros((config['num_classes'], 3), dtype=torch.int64, device=next(model.parameters()).device)
            hist = evaluate_image(model, image, label, config, batch_size, dedupe, precision, counts, tta, True if hist is None else hist)
        else:
            counts = evaluate_image(model, image, label, config, batch_size, dedupe, precision, counts, tta)
    if counts is None:
        raise ValueError('evaluate_images: no (image, label) pair given')
    counts = counts.cpu().numpy()
    smooth = 1e-5
    iou = [float((i + smooth) / (p + g - i + smooth)) for i, p, g in counts.tolist()]
    dice = [float((2 * i + smooth) / (p + g + smooth)) for i, p, g in counts.tolist()]
    res = dict(counts=counts, iou=iou, dice=dice)
    if sweep:
        res['hist'] = hist.cpu().numpy()
        res.update(threshold_curves(res['hist']))
    return res


def load_segmentation_models(config_file):
    """api.py:302-333: read <model_path>/<name>/config.yml, build archs[config['arch']], load model.pth, eval mode; force
    patch_size 1024 and take patch_overlap from val_config."""
    import yaml
    config_dict = json.loads(open(config_file, 'rt').read())
    file_dict, val_config = config_dict['file_path'], config_dict['val_config']
    model_folder, name = file_dict['model_path'], val_config['name']
    with open(os.path.join(model_folder, '%s/config.yml' % name), 'r') as f:
        config = yaml.load(f, Loader=yaml.FullLoader)
    config['name'] = name
    print('-' * 20)
    for key in config.keys():
        print('%s: %s' % (key, str(config[key])))
    print('-' * 20)
    print("=> creating model %s" % config['arch'])
    if config['arch'] not in archs.__all__:
        raise NotImplementedError('arch %r is not built in ssunet-gan_amd' % config['arch'])
    model = archs.__dict__[config['arch']](config['num_classes'], config['input_channels'], config['deep_supervision'])
    model = model.cuda()
    state = torch.load(os.path.join(model_folder, '%s/model.pth' % config['name']), map_location='cpu')
    model.load_state_dict(state)
    model.eval()
    config['patch_size'] = 1024
    config['patch_overlap'] = val_config['patch_overlap']
    return model, config


def segmentation_inference_full(model, img_input, img_patch_set, mask_patch_set, config, gt_mask_flag, batch_size=12, precision='fp32'):
    """api.py:376-410 complete: (all_class_mask, gt_class_mask) as lists of uint8 {0, 255} masks at image resolution.  The model
    forward is batched (`batch_size` patches per launch sequence; 1 = the reference's loop).  `precision`: see `infer_patches`
    ('bf16x1' is an approximation with bf16 operand rounding in the BasicBlock 3x3 stride-1 convs)."""
    patch_size, infer_size, p_overlap = config['patch_size'], config['input_w'], config['patch_overlap']
    full_output = list(infer_patches(model, img_patch_set, batch_size, precision=precision).numpy())
    all_class_mask = patch_merge(img_input, full_output, patch_size, config, p_overlap)
    if gt_mask_flag is True:
        gt_label = []
        for data in mask_patch_set:
            m = np.dstack([mask_convert(data, c, infer_size) for c in range(config['num_classes'])]).transpose(2, 0, 1)
            gt_label.append(m / 255.0)
        gt_class_mask = patch_merge(img_input, gt_label, patch_size, config, p_overlap)
    else:
        gt_class_mask = all_class_mask
    return all_class_mask, gt_class_mask
