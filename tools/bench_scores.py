"""What the confidence maps cost, one JSON object per line: one 2048^2 random image, patch 1024 -> 512, overlap 0.5
(BASELINE config 5), the probabilities those of the seeded generator.  Rows: `ssg_sw_merge_masks_f32_u8` (the yardstick), mask mode
and score mode of `ssg_sw_merge_scores_f32_u8` on the same operands by HIP events, alternated round by round in one process, for
the 9 unique and all 36 patches, and for the 100 patches of overlap 0.75 (64 voters on a pixel: the score kernel's overflow path);
`ssg_sw_score_hist_u8` with its algorithmic bytes as a fraction of the copy rate `bench.py --full`
reports (the same 1 GiB -> 1 GiB copy, measured in this run), on the model's scores and on a flat map; `segment_image` /
`evaluate_image` with and without the new keywords.  `--segment-only TAG` times `segment_image` with every keyword at its default
and nothing else: the row to take from an export of the parent commit and from this tree, alternated in one job.
Not the graded metric (bench.py).  Usage (GPU box): python tools/bench_scores.py [--out FILE.jsonl] [--segment-only TAG]"""
import argparse
import ctypes
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


def alternated(fns, rounds, n):
    """{name: (median ms, min, max over the rounds)}: every round times each fn once (n launches by HIP events), in list order."""
    ms = {name: [] for name, _ in fns}
    for r in range(rounds):
        for name, fn in fns:
            ms[name].append(event_ms(fn, 5 if r == 0 else 1, n))
    return {name: (sorted(v)[len(v) // 2], min(v), max(v)) for name, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None, help='also write (append) the rows to this .jsonl file')
    ap.add_argument('--segment-only', default=None, metavar='TAG', help='only time segment_image at its defaults; TAG names the tree')
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

    def finish():
        if args.out:
            with open(args.out, 'a') as f:
                for r in rows:
                    f.write(json.dumps(r) + '\n')

    if args.segment_only:
        row = {'tree': args.segment_only, 'what': 'segment_image with every keyword at its default, 2048^2, patch 1024 -> 512, batch 12, '
                                                  '(mean, min, max) of 10 calls after a warm-up, wall s'}
        for dedupe in (True, False):
            row['fp32_dedupe' if dedupe else 'fp32_all_36'] = [round(v, 5) for v in timed(
                lambda: A.segment_image(G, img, cfg, batch_size=12, dedupe=dedupe), 1, 10)]
        emit(row)
        return finish()

    # the three merges on the same operands, alternated; the last case is the other side of the score kernel's choice: overlap 0.75
    # without dedupe puts 64 patches on an interior pixel, more than the pair cache holds, so those waves bisect over the patch list
    for dedupe in (True, False, None):
        if dedupe is None:
            org = A.patch_origins(H, W, P_SIZE, 0.75)
            wts = [1] * len(org)
            probs = ops.new_nhwc(len(org), 3, SIZE, SIZE, dev)
            probs.copy_(torch.rand((len(org), 3, SIZE, SIZE), device=dev, generator=torch.Generator(device=dev).manual_seed(5)))
        else:
            _, _, probs, org, wts, _ = A._device_masks(G, img, cfg, 12, dedupe, 'fp32', None, 'bench_scores')
        host, devo = ops._sw_origins(org, dev)
        wdev = torch.as_tensor(wts, dtype=torch.int32).to(dev)
        n, ld = len(org), ops.nhwc_ld(probs)
        outs = [torch.empty((3, H, W), dtype=torch.uint8, device=dev) for _ in range(3)]
        lv = (ctypes.c_int32 * 3)(127, 127, 127)
        fns = [('merge_masks', lambda: L.call('ssg_sw_merge_masks_f32_u8', L.ptr(probs), ld, n, 3, SIZE, L.ptr(devo), L.ptr(host), L.ptr(wdev),
                                              P_SIZE, H, W, L.ptr(outs[0]), L.stream_ptr())),
               ('mask_mode', lambda: L.call('ssg_sw_merge_scores_f32_u8', L.ptr(probs), ld, n, 3, SIZE, L.ptr(devo), L.ptr(host), L.ptr(wdev),
                                            P_SIZE, H, W, lv, L.ptr(outs[1]), L.stream_ptr())),
               ('score_mode', lambda: L.call('ssg_sw_merge_scores_f32_u8', L.ptr(probs), ld, n, 3, SIZE, L.ptr(devo), L.ptr(host), L.ptr(wdev),
                                             P_SIZE, H, W, None, L.ptr(outs[2]), L.stream_ptr()))]
        ms = alternated(fns, 5, 200) if dedupe is not None else alternated(fns, 3, 50)
        sc = outs[2]
        emit({'what': 'merge kernels alone on %s, %d patches (%s): %s, alternated, HIP events, ms (median, min, max over the rounds)'
                      % ('uniform random probabilities' if dedupe is None else 'the generator\'s probabilities', n,
                         'overlap 0.75, all origins, weights 1, up to 64 on a pixel' if dedupe is None else
                         'unique origins, weights 4' if dedupe else 'all origins, weights 1',
                         '3 rounds of 50 launches each' if dedupe is None else '5 rounds of 200 launches each'),
              'patches': n,
              **{'ms_' + k: [round(x, 4) for x in v] for k, v in ms.items()},
              'mask_mode_over_merge_masks': round(ms['mask_mode'][0] / ms['merge_masks'][0], 3),
              'score_mode_over_merge_masks': round(ms['score_mode'][0] / ms['merge_masks'][0], 3),
              'mask_mode_equals_merge_masks': bool(torch.equal(outs[1], outs[0])),
              'scores_above_127_equal_merge_masks': bool(torch.equal((sc > 127).to(torch.uint8) * 255, outs[0])),
              'distinct_score_values': int(torch.unique(sc).numel())})
        if dedupe is not True:
            continue
        # the histogram on these scores and on a flat map, against the copy rate
        tbps = copy_tbps()
        gt = A._device_masks(G, img, cfg, 12, True, 'fp32', lab, 'bench_scores')[1]
        flat = ((torch.arange(H * W, device=dev) // 4096) % 2 * 255).to(torch.uint8).repeat(3).view(3, H, W).contiguous()
        hrow = {'what': 'score histogram alone (HIP events, 1000 launches, operands resident), algorithmic bytes (scores + ground truth) '
                        'against the 1 GiB copy rate of this run', 'hbm_copy_tbps': round(tbps, 2), 'bytes': 2 * 3 * H * W}
        for name, scores in (('model_scores', sc), ('flat_runs_of_4096', flat)):
            hist = torch.zeros((3, 2, 256), dtype=torch.int64, device=dev)
            ms_h = event_ms(lambda: L.call('ssg_sw_score_hist_u8', L.ptr(scores), L.ptr(gt), 3, H * W, L.ptr(hist), L.stream_ptr()), 10, 1000)
            want = A.score_hist(scores.cpu().numpy(), gt.cpu().numpy())
            hrow['ms_hist_' + name] = round(ms_h, 4)
            hrow['hist_%s_tb_per_s' % name] = round(2 * 3 * H * W / ms_h / 1e9, 3)
            hrow['hist_%s_fraction_of_copy' % name] = round(2 * 3 * H * W / ms_h / 1e9 / tbps, 3)
            hrow['hist_%s_after_1010_launches_equals_1010_x_host' % name] = bool(np.array_equal(hist.cpu().numpy(), 1010 * want))
        counts = torch.zeros((3, 3), dtype=torch.int64, device=dev)
        hrow['ms_mask_counts_same_operands'] = round(event_ms(
            lambda: L.call('ssg_sw_mask_counts_u8', L.ptr(sc), L.ptr(gt), 3, H * W, L.ptr(counts), L.stream_ptr()), 10, 1000), 4)
        emit(hrow)

    # the calls: defaults against the new keywords, alternated
    for dedupe in (True, False):
        calls = [('default', lambda: A.segment_image(G, img, cfg, batch_size=12, dedupe=dedupe)),
                 ('threshold_127', lambda: A.segment_image(G, img, cfg, batch_size=12, dedupe=dedupe, threshold=127)),
                 ('return_scores', lambda: A.segment_image(G, img, cfg, batch_size=12, dedupe=dedupe, return_scores=True))]
        acc = {k: [] for k, _ in calls}
        for r in range(2):
            for k, fn in calls:
                acc[k].append(timed(fn, 1 if r == 0 else 0, 5))
        emit({'what': 'segment_image (batch 12, %s), wall s (mean, min, max) of 2 x 5 calls, the three forms alternated; return_scores '
                      'also downloads 12 MiB of scores' % ('dedupe' if dedupe else 'all 36 patches'),
              **{'s_' + k: [round(sum(t[0] for t in v) / len(v), 5), round(min(t[1] for t in v), 5), round(max(t[2] for t in v), 5)]
                 for k, v in acc.items()}})
    ev = [('evaluate_image', lambda: A.evaluate_image(G, img, lab, cfg, batch_size=12)),
          ('evaluate_image_hist', lambda: A.evaluate_image(G, img, lab, cfg, batch_size=12, hist=True))]
    acc = {k: [] for k, _ in ev}
    for r in range(2):
        for k, fn in ev:
            acc[k].append(timed(fn, 1 if r == 0 else 0, 5))
    res = A.evaluate_images(G, [(img, lab)], cfg, batch_size=12, sweep=True)
    plain = A.evaluate_images(G, [(img, lab)], cfg, batch_size=12)
    emit({'what': 'evaluate_image (dedupe, batch 12) without / with hist=True, wall s (mean, min, max) of 2 x 5 calls alternated; and one '
                  'evaluate_images(sweep=True) on the pair (a random-weight generator: the numbers say nothing about a trained model)',
          **{'s_' + k: [round(sum(t[0] for t in v) / len(v), 5), round(min(t[1] for t in v), 5), round(max(t[2] for t in v), 5)]
             for k, v in acc.items()},
          'sweep_counts_equal_plain_counts': bool(np.array_equal(res['counts'], plain['counts'])),
          'iou_at_127': [round(v, 6) for v in res['iou']], 'best_threshold': res['best_threshold'],
          'best_iou': [round(v, 6) for v in res['best_iou']]})
    finish()


if __name__ == '__main__':
    main()
