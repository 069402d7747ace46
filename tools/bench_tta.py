"""What flip / rotation test-time augmentation costs, one JSON object per line: one 2048^2 random image, patch
1024 -> 512, overlap 0.5 (BASELINE config 5), seeded UNet_R_SS_v2.
Rows: wall time of `segment_image` for tta in None, 'hflip', 'flips', 'd4' with `dedupe` on and off and precision 'fp32' and
'bf16x1', each beside K x the tta=None time of the same settings in the same run (tta=None runs the statements the pipeline had
before `tta` existed) and what exceeds it; then the two kernels alone by HIP events -- one oriented gather per code, the reduce per
K with even (r = 0, 2: read along rows) and odd (r = 1, 3: transposed through LDS) codes apart -- with the reduce's algorithmic
bytes per second against `ssg_tool_copy_f32` on the same number of bytes and on 1 GiB, measured in this process.
No accuracy is measured: there is no trained checkpoint.  Not the graded metric (bench.py).
Usage (GPU box): python tools/bench_tta.py [--out FILE.jsonl] [--reps N]"""
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
P_SIZE, SIZE = 1024, 512


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


def copy_tbps(nbytes_moved):
    """ssg_tool_copy_f32 moving `nbytes_moved` in all (half read, half written), TB/s."""
    L = S._lib
    n = max(nbytes_moved // 8 // 4 * 4, 4)
    a = torch.empty(n, device=dev)
    b = torch.empty(n, device=dev)
    ms = event_ms(lambda: L.call('ssg_tool_copy_f32', L.ptr(a), L.ptr(b), n, L.stream_ptr()), 3, 20 if n < (1 << 27) else 3)
    return 2 * n * 4 / ms / 1e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None, help='also write the rows to this .jsonl file')
    ap.add_argument('--reps', type=int, default=3, help='timed segment_image calls per setting')
    args = ap.parse_args()
    A, ops, L = S.aerial_image_segmentation_api, S.ops, S._lib
    cfg = dict(patch_size=P_SIZE, input_w=SIZE, input_h=SIZE, patch_overlap=0.5, num_classes=3)
    img = np.random.default_rng(5).integers(0, 256, (H, W, 3), dtype=np.uint8)
    torch.manual_seed(41)
    G = S.models_seg_gan.Generator(dict(arch='UNet_R_SS_v2', num_classes=3, input_channels=3, deep_supervision=False)).to(dev).eval()
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    for precision in ('fp32', 'bf16x1'):
        for dedupe in (True, False):
            base = None
            for tta in (None, 'hflip', 'flips', 'd4'):
                k = len(ops.tta_codes(tta))
                t = timed(lambda: A.segment_image(G, img, cfg, batch_size=12, dedupe=dedupe, precision=precision, tta=tta), 1, args.reps)
                if tta is None:
                    base = t[0]
                emit({'what': 'segment_image, one 2048^2 image, patch 1024 -> 512, overlap 0.5, batch 12', 'precision': precision,
                      'dedupe': dedupe, 'tta': tta, 'views': k, 's': round(t[0], 5), 's_min_max': [round(t[1], 5), round(t[2], 5)],
                      's_views_x_tta_none': round(k * base, 5), 's_beyond_views_x_tta_none': round(t[0] - k * base, 5),
                      'ratio_to_views_x_tta_none': round(t[0] / (k * base), 3)})

    # the two kernels alone: the 9 distinct origins of the image (one dedupe batch)
    org = A.unique_origins(A.patch_origins(H, W, P_SIZE, 0.5))[0]
    n = len(org)
    dimg = torch.from_numpy(img).to(dev)
    host, devo = ops._sw_origins(org, dev)
    norm = ops._sw_norm_consts()
    out = ops.new_nhwc(n, 3, SIZE, SIZE, dev)
    grow = {'what': 'one gather of %d patches 1024 -> 512 per D4 code (HIP events, 200 launches); code 0 is ssg_sw_gather_patches_u8_f32, '
                    'the others ssg_sw_gather_patches_d4_u8_f32; bytes = 3 p^2 read + 16 s^2 written per patch' % n,
            'bytes': n * (3 * P_SIZE * P_SIZE + 16 * SIZE * SIZE)}
    grow['ms_code_0_plain_entry'] = round(event_ms(lambda: L.call('ssg_sw_gather_patches_u8_f32', L.ptr(dimg), H, W, L.ptr(devo), L.ptr(host), n,
                                                                   P_SIZE, SIZE, *(norm + [L.ptr(out), L.stream_ptr()])), 10, 200), 4)
    for code in range(8):
        grow['ms_code_%d' % code] = round(event_ms(
            lambda: L.call('ssg_sw_gather_patches_d4_u8_f32', L.ptr(dimg), H, W, L.ptr(devo), L.ptr(host), n, P_SIZE, SIZE, code,
                           *(norm + [L.ptr(out), L.stream_ptr()])), 10, 200), 4)
    emit(grow)

    copy_1g = copy_tbps(2 << 30)
    stack = ops.new_tta_stack(8, n, 3, SIZE, dev)
    stack.copy_(torch.rand(8, n, 3, SIZE, SIZE, device=dev))
    res = ops.new_nhwc(n, 3, SIZE, SIZE, dev)
    for codes, kind in (((0,), 'even'), ((1,), 'odd'), ((0, 4), 'even'), ((1, 3), 'odd'), ((0, 4, 2, 6), 'even'), ((1, 3, 5, 7), 'odd'),
                        ((0, 1, 2, 3), 'half odd'), (tuple(range(8)), 'half odd')):
        k = len(codes)
        assert torch.equal(ops.sw_tta_reduce(stack[:k], codes), ops.sw_tta_reduce(stack[:k], codes, out=res))
        host_codes = (ctypes.c_int32 * k)(*codes)
        ms = event_ms(lambda: L.call('ssg_sw_tta_reduce_f32', L.ptr(stack), stack.stride(0), 4, k, host_codes, n, 3, SIZE, L.ptr(res), 4,
                                     L.stream_ptr()), 10, 200)
        nbytes = (k + 1) * n * SIZE * SIZE * 16
        same = copy_tbps(nbytes)
        emit({'what': 'ssg_sw_tta_reduce_f32 on [K, %d, 3, 512, 512] (HIP events, 200 launches); bytes = (K + 1) '
                      'views of 16 B pixels; copy = ssg_tool_copy_f32 in this process' % n,
              'views': k, 'codes': list(codes), 'rotations': kind, 'ms': round(ms, 4), 'bytes': nbytes, 'tb_per_s': round(nbytes / ms / 1e9, 3),
              'copy_same_bytes_tb_per_s': round(same, 3), 'fraction_of_copy_same_bytes': round(nbytes / ms / 1e9 / same, 3),
              'copy_1gib_tb_per_s': round(copy_1g, 3), 'fraction_of_copy_1gib': round(nbytes / ms / 1e9 / copy_1g, 3)})
    if args.out:
        with open(args.out, 'w') as f:
            for r in rows:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
