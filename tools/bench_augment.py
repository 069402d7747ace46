"""What the device-side training augmentation costs, one JSON object per line: batches of 16 tiles to 512^2,
C = 3 mask channels, from 512^2 and from 1024^2 uint8 sources, parameters drawn by augment.sample_params (seed 0).
Rows, per source size:
  host: tests/augment_ref.py (the numpy definition) on the same batch, on one core and as 16 processes, one sample each at a time;
        taken first, before this process touches the GPU;
  kernel: ssg_augment_batch_u8_f32 by HIP events, its algorithmic bytes (every source byte once, 32 B written per output pixel)
        per second, beside a hipMemcpyAsync device-to-device copy (Tensor.copy_) moving the same number of bytes in this process;
  call: ops.augment_batch as the trainer calls it (tables uploaded, outputs allocated), wall time with a synchronise.
Then the G+D step at 16 x 512^2 (UNet_R_SS_v2 + Discriminator, fp32), alternated in this process, fed by (a) an fp32 NCHW batch
uploaded from pageable host memory as train() does today and (b) uint8 NHWC tiles uploaded and passed through DeviceAugment.
No accuracy is measured: there is no trained checkpoint.  Not the graded metric (bench.py).
Usage (GPU box): python tools/bench_augment.py [--out FILE.jsonl] [--steps N]"""
import argparse
import json
import multiprocessing
import os
import sys
import time

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import augment_ref as ar  # noqa: E402
import ssunet_gan_amd as S  # noqa: E402

N, OUT, C = 16, 512, 3
CONFIG = dict(rotate_min=-10, rotate_max=10, input_h=OUT, input_w=OUT)


def batch(src):
    g = np.random.default_rng(5)
    img = g.integers(0, 256, (N, src, src, 3), dtype=np.uint8)
    mask = g.integers(0, 2, (N, src, src, C), dtype=np.uint8)
    params, luts = S.augment.sample_params(N, (src, src), (OUT, OUT), CONFIG, np.random.default_rng(0))
    return img, mask, params, luts


def _one(args):
    ar.augment_one(*args)
    return 0


def host_seconds(img, mask, params, luts, procs):
    jobs = [(img[k], mask[k], params[k], luts[k], OUT, OUT) for k in range(N)]
    if procs == 1:
        t0 = time.perf_counter()
        for j in jobs:
            _one(j)
        return time.perf_counter() - t0
    with multiprocessing.get_context('fork').Pool(procs) as pool:
        pool.map(_one, jobs[:procs])                         # workers started and warm
        t0 = time.perf_counter()
        pool.map(_one, jobs, chunksize=1)
        return time.perf_counter() - t0


def event_ms(fn, warm, n):
    for _ in range(warm):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def wall_ms(fn, warm, n):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None, help='also write the rows to this .jsonl file')
    ap.add_argument('--steps', type=int, default=6, help='timed G+D steps per arm and round')
    args = ap.parse_args()
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    data = {src: batch(src) for src in (512, 1024)}
    for src in (512, 1024):                                  # host first: forked workers must not inherit an initialised GPU
        one = host_seconds(*data[src], procs=1)
        many = host_seconds(*data[src], procs=16)
        emit({'what': 'tests/augment_ref.py (numpy) on the host, %d x %d^2 -> %d^2, C = %d' % (N, src, OUT, C), 'src': src,
              's_one_core': round(one, 3), 's_16_processes': round(many, 3),
              'images_per_s_one_core': round(N / one, 1), 'images_per_s_16_processes': round(N / many, 1)})

    dev = torch.device('cuda')
    L, ops = S._lib, S.ops
    norm = ops._sw_norm_consts()
    for src in (512, 1024):
        img, mask, params, luts = data[src]
        gi, gm = torch.from_numpy(img).to(dev), torch.from_numpy(mask).to(dev)
        hp, gl = torch.from_numpy(params), torch.from_numpy(luts).to(dev)
        gp = hp.to(dev)
        oi, ot = ops.new_nhwc(N, 3, OUT, OUT, dev), ops.new_nhwc(N, C, OUT, OUT, dev)
        ms = event_ms(lambda: L.call('ssg_augment_batch_u8_f32', L.ptr(gi), L.ptr(gm), N, src, src, C, L.ptr(gp), L.ptr(hp), L.ptr(gl), OUT, OUT,
                                     0, 0, 0, *(norm + [L.ptr(oi), L.ptr(ot), L.stream_ptr()])), 10, 200)
        nbytes = N * src * src * (3 + C) + N * OUT * OUT * 32
        a = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
        b = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
        cp = event_ms(lambda: b.copy_(a), 10, 200)
        call = wall_ms(lambda: ops.augment_batch(gi, gm, params, luts, OUT, OUT), 5, 50)
        emit({'what': 'ssg_augment_batch_u8_f32, %d x %d^2 -> %d^2, C = %d (HIP events, 200 launches); bytes = every source byte once + 32 B '
                      'per output pixel; copy = hipMemcpyAsync device to device moving the same bytes (half read, half written)' % (N, src, OUT, C),
              'src': src, 'kernel_ms': round(ms, 4), 'bytes': nbytes, 'tb_per_s': round(nbytes / ms / 1e9, 3),
              'bytes_per_output_pixel': round(nbytes / (N * OUT * OUT), 1),
              'copy_same_bytes_ms': round(cp, 4), 'copy_same_bytes_tb_per_s': round(nbytes / cp / 1e9, 3), 'kernel_over_copy': round(ms / cp, 3),
              'ops_augment_batch_wall_ms_median_min_max': [round(float(np.median(call)), 4), round(min(call), 4), round(max(call), 4)]})

    # the G+D step, two ways of feeding it, alternated
    torch.manual_seed(41)
    G = S.models_seg_gan.Generator(dict(arch='UNet_R_SS_v2', num_classes=3, input_channels=3, deep_supervision=False)).to(dev).train()
    D = S.models_seg_gan.Discriminator(3, kernel_size=3, n_channels=64, n_blocks=8, fc_size=1024).to(dev).train()
    og, od = torch.optim.Adam(G.parameters(), lr=2e-5), torch.optim.Adam(D.parameters(), lr=2e-5)
    crit, adv, con = S.losses.BCEDiceLoss(), nn.BCEWithLogitsLoss(), nn.MSELoss()
    img, mask, _, _ = data[512]
    u8_img, u8_mask = torch.from_numpy(img), torch.from_numpy(mask)
    aug = S.augment.DeviceAugment(CONFIG, seed=0)
    fi, ft = aug(u8_img.to(dev), u8_mask.to(dev))
    f32_img, f32_tgt = fi.contiguous().cpu(), ft.contiguous().cpu()             # what a host pipeline hands over: fp32 NCHW
    assert f32_img.is_contiguous() and f32_img.shape == (N, 3, OUT, OUT)

    def step_f32():
        S.train_seg_gan.gan_step(f32_img.cuda(non_blocking=True), f32_tgt.cuda(non_blocking=True), G, D, crit, adv, con, og, od, 3)

    def step_u8():
        inp, tgt = aug(u8_img.cuda(non_blocking=True), u8_mask.cuda(non_blocking=True))
        S.train_seg_gan.gan_step(inp, tgt, G, D, crit, adv, con, og, od, 3)

    arms = (('fp32_nchw_upload', step_f32), ('uint8_upload_device_augment', step_u8))
    for _, fn in arms:
        wall_ms(fn, 2, 1)
    res = {k: [] for k, _ in arms}
    for _ in range(2):
        for k, fn in arms:
            res[k].append(round(float(np.median(wall_ms(fn, 1, args.steps))), 3))
    emit({'what': 'G+D step at %d x %d^2, fp32, fed two ways, alternated twice in one process: median wall ms per step (upload + step, '
                  'synchronised) of %d steps per round; upload bytes per batch' % (N, OUT, args.steps),
          'ms_per_step_rounds': res, 'images_per_s': {k: round(N / (np.mean(v) / 1e3), 2) for k, v in res.items()},
          'upload_bytes': {'fp32_nchw_upload': f32_img.numel() * 4 + f32_tgt.numel() * 4,
                           'uint8_upload_device_augment': u8_img.numel() + u8_mask.numel() + N * (64 + 256)}})
    if args.out:
        with open(args.out, 'w') as f:
            for r in rows:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
