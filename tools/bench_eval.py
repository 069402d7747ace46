"""What the device-side ground-truth branch and evaluation cost, one JSON object per line: one 2048^2 random
image with a label of 16-pixel palette blocks, patch 1024 -> 512, overlap 0.5 (BASELINE config 5 with gt_mask_flag on).
Rows: the host ground-truth branch (mask_convert x 108 + patch_merge), `segment_image` with and without `label_bgr` for both
`dedupe` settings, `evaluate_image`, and the two kernels alone by HIP events with their algorithmic bytes as a fraction of the
copy rate `bench.py --full` reports (the same 1 GiB -> 1 GiB copy, measured in this run).  Not the graded metric (bench.py).
Usage (GPU box): python tools/bench_eval.py [--out FILE.jsonl]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ssunet_gan_amd as S  # noqa: E402

dev = torch.device('cuda')
H = W = 2048
P_SIZE, SIZE, BLOCK = 1024, 512, 16
PALETTE = np.array([(255, 255, 255), (255, 0, 0), (0, 0, 255), (0, 255, 0)], dtype=np.uint8)   # three classes and background


def timed(fn, warm, n):
    """(mean, min, max) wall seconds of fn(), synchronised."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return sum(ts) / n, min(ts), max(ts)


def event_ms(fn, warm, n):
    """HIP-event time of one fn() in ms (fn only enqueues)."""
    for _ in range(warm):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def copy_tbps():
    """The HBM copy rate as bench.py --full measures it: ssg_tool_copy_f32, 1 GiB -> 1 GiB."""
    L = S._lib
    a = torch.empty(1 << 28, device=dev)
    b = torch.empty(1 << 28, device=dev)
    ms = event_ms(lambda: L.call('ssg_tool_copy_f32', L.ptr(a), L.ptr(b), a.numel(), L.stream_ptr()), 1, 3)
    return 2 * a.numel() * 4 / ms / 1e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None, help='also write the rows to this .jsonl file')
    args = ap.parse_args()
    A, ops, L = S.aerial_image_segmentation_api, S.ops, S._lib
    cfg = dict(patch_size=P_SIZE, input_w=SIZE, input_h=SIZE, patch_overlap=0.5, num_classes=3)
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    idx = rng.integers(0, len(PALETTE), (H // BLOCK, W // BLOCK))
    lab = np.ascontiguousarray(PALETTE[np.repeat(np.repeat(idx, BLOCK, 0), BLOCK, 1)])
    torch.manual_seed(41)
    G = S.models_seg_gan.Generator(dict(arch='UNet_R_SS_v2', num_classes=3, input_channels=3, deep_supervision=False)).to(dev).eval()
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    # the host ground-truth branch of segmentation_inference_full: mask_convert per patch and class, then patch_merge
    def host_gt():
        _, mask_patch = A.patch_gen(lab, lab, P_SIZE, 0.5)
        gt = [np.dstack([A.mask_convert(p, c, SIZE) for c in range(3)]).transpose(2, 0, 1) / 255.0 for p in mask_patch]
        return A.patch_merge(lab, gt, P_SIZE, cfg, 0.5)
    t0 = time.perf_counter()
    want_gt = host_gt()
    t_host = time.perf_counter() - t0
    row = {'what': 'ground-truth branch of one 2048^2 label image (16-px palette blocks), patch 1024 -> 512, overlap 0.5: host '
                   'mask_convert x 108 + patch_merge, against segment_image with / without label_bgr (batch 12, same process)',
           's_host_gt_branch': round(t_host, 3)}
    same = True
    for dedupe in (False, True):
        tag = 'dedupe' if dedupe else 'all_36'
        # alternate the two forms so that clock drift lands on both
        t_without = timed(lambda: A.segment_image(G, img, cfg, batch_size=12, dedupe=dedupe), 1, 5)
        t_with = timed(lambda: A.segment_image(G, img, cfg, batch_size=12, dedupe=dedupe, label_bgr=lab), 1, 5)
        t_without2 = timed(lambda: A.segment_image(G, img, cfg, batch_size=12, dedupe=dedupe), 0, 5)
        t_with2 = timed(lambda: A.segment_image(G, img, cfg, batch_size=12, dedupe=dedupe, label_bgr=lab), 0, 5)
        without = (t_without[0] + t_without2[0]) / 2
        with_ = (t_with[0] + t_with2[0]) / 2
        row['s_segment_image_%s' % tag] = round(without, 5)
        row['s_segment_image_%s_min_max' % tag] = [round(min(t_without[1], t_without2[1]), 5), round(max(t_without[2], t_without2[2]), 5)]
        row['s_segment_image_%s_with_label' % tag] = round(with_, 5)
        row['s_segment_image_%s_with_label_min_max' % tag] = [round(min(t_with[1], t_with2[1]), 5), round(max(t_with[2], t_with2[2]), 5)]
        row['s_added_by_label_%s' % tag] = round(with_ - without, 5)
        row['host_gt_branch_over_added_%s' % tag] = round(t_host / max(with_ - without, 1e-9), 1)
        _, got_gt = A.segment_image(G, img, cfg, batch_size=12, dedupe=dedupe, label_bgr=lab)
        same = same and all(np.array_equal(a, b) for a, b in zip(got_gt, want_gt))
    row['gt_masks_equal_host'] = bool(same)
    emit(row)

    t_eval = timed(lambda: A.evaluate_image(G, img, lab, cfg, batch_size=12), 1, 5)
    masks, gt = A.segment_image(G, img, cfg, batch_size=12, label_bgr=lab)
    host_counts = [[int(((m > 127) & (g > 127)).sum()), int((m > 127).sum()), int((g > 127).sum())] for m, g in zip(masks, gt)]
    res = A.evaluate_images(G, [(img, lab)], cfg, batch_size=12)
    emit({'what': 'evaluate_image on the same pair (dedupe, batch 12): both mask sets stay on the device, 72 bytes of counts come back',
          's_evaluate_image': round(t_eval[0], 5), 's_evaluate_image_min_max': [round(t_eval[1], 5), round(t_eval[2], 5)],
          'counts': res['counts'].tolist(), 'counts_equal_host': res['counts'].tolist() == host_counts,
          'iou': [round(v, 6) for v in res['iou']], 'dice': [round(v, 6) for v in res['dice']]})

    # the two kernels alone
    tbps = copy_tbps()
    dlab = torch.from_numpy(lab).to(dev)
    krow = {'what': 'label gather and mask counts alone (HIP events, 1000 launches, operands resident), algorithmic bytes against the '
                    '1 GiB copy rate of this run', 'hbm_copy_tbps': round(tbps, 2)}
    for name, org in (('36', A.patch_origins(H, W, P_SIZE, 0.5)), ('9', A.unique_origins(A.patch_origins(H, W, P_SIZE, 0.5))[0])):
        host, devo = ops._sw_origins(org, dev)
        n = len(org)
        out = ops.new_nhwc(n, 3, SIZE, SIZE, dev)
        ms = event_ms(lambda: L.call('ssg_sw_gather_labels_u8_f32', L.ptr(dlab), H, W, L.ptr(devo), L.ptr(host), n, P_SIZE, SIZE, 3,
                                     L.ptr(out), L.stream_ptr()), 10, 1000)
        nbytes = n * (3 * P_SIZE * P_SIZE + 16 * SIZE * SIZE)
        krow['ms_gather_labels_%s_patches' % name] = round(ms, 4)
        krow['gather_labels_%s_bytes' % name] = nbytes
        krow['gather_labels_%s_tb_per_s' % name] = round(nbytes / ms / 1e9, 3)
        krow['gather_labels_%s_fraction_of_copy' % name] = round(nbytes / ms / 1e9 / tbps, 3)
        del out
    pred = torch.from_numpy(np.stack(masks)).to(dev)
    gtd = torch.from_numpy(np.stack(gt)).to(dev)
    counts = torch.zeros((3, 3), dtype=torch.int64, device=dev)
    ms = event_ms(lambda: L.call('ssg_sw_mask_counts_u8', L.ptr(pred), L.ptr(gtd), 3, H * W, L.ptr(counts), L.stream_ptr()), 10, 1000)
    nbytes = 2 * 3 * H * W
    krow.update({'ms_mask_counts': round(ms, 4), 'mask_counts_bytes': nbytes, 'mask_counts_tb_per_s': round(nbytes / ms / 1e9, 3),
                 'mask_counts_fraction_of_copy': round(nbytes / ms / 1e9 / tbps, 3),
                 'counts_after_1010_launches_equal_1010_x_host': counts.cpu().numpy().tolist() == (1010 * np.array(host_counts)).tolist()})
    emit(krow)
    if args.out:
        with open(args.out, 'w') as f:
            for r in rows:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
