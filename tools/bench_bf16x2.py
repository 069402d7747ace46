"""Opt-in precision 'bf16x2', measured.  Everything in one process on one box, the three precisions alternated over
ROUNDS rounds, HIP events, random operands; one JSON line per row:

  fwd        per BasicBlock 3x3 shape of UNet_R_SS_v2 at N x 512^2 (N = 16): ops._conv_fwd_impl under 'fp32' (conv_halo_k32, or
             whatever the plan picks), 'bf16x1' (conv_halo_k32_x1_kernel) and 'bf16x2' (conv_halo_k32_x2_kernel);
  dgrad      the same shapes: ops._conv_dgrad_impl under the three precisions, per input pointer of a concat conv;
  wgrad      the same shapes: ops._conv_wgrad_impl under the three precisions;
  generator  forward + backward of the generator (train-mode batch norm) under train_precision 'fp32' / 'bf16x1' / 'bf16x2';
  gan_step   the full G+D step under the three values of `precision`;
  segment    segment_image on one 2048^2 image (patch 1024, overlap 0.5, inference at 512^2, batch 12) per precision.

`route` = the two-term kernel was faster than the fp32-class kernel in this run: the rule by which a shape may stay in the bf16x2
predicates.  No speed-up is promised: the tool states what comes out.
Usage: python tools/bench_bf16x2.py [--out file] [--only fwd,dgrad,wgrad,generator,gan_step,segment]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ssunet_gan_amd as S                                                    # noqa: E402
from ssunet_gan_amd import ops                                                # noqa: E402

MODES = ('fp32', 'bf16x1', 'bf16x2')
# (C1, C2, Cout, size at 512^2 input): conv1 (encoder, and decoder with the concat) and conv2 of every BasicBlock that is >= 17 wide
SHAPES = [(64, 0, 64, 512), (64, 128, 64, 512), (64, 0, 128, 256), (128, 0, 128, 256), (128, 256, 128, 256), (128, 0, 256, 128),
          (256, 0, 256, 128), (256, 256, 256, 128), (256, 0, 384, 64), (384, 0, 384, 64), (384, 384, 384, 64), (384, 0, 512, 32),
          (512, 0, 512, 32), (512, 512, 512, 32)]


def timed(fn, reps):
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def label_of(fn):
    ops.PROFILE = []
    try:
        fn()
        torch.cuda.synchronize()
        return [r[0] for r in ops.PROFILE][0]
    finally:
        ops.PROFILE = None


def alternate(fns, reps, rounds):
    for fn in fns.values():
        timed(fn, 2)
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            ms[k].append(timed(fn, reps))
    return ms


def layer_row(kind, shape, n, flops, make, rounds, extra=None):
    """make(mode) -> a launch under that precision."""
    fns = {m: make(m) for m in MODES}
    reps = max(4, int(1e12 / flops))
    ms = alternate(fns, reps, rounds)
    t = {m: min(ms[m]) for m in MODES}
    row = dict(bench=kind, shape=shape, batch=n)
    for m in MODES:
        row['kernel_' + m] = label_of(fns[m])
        row['ms_' + m] = round(t[m], 4)
        row['tflops_' + m] = round(flops / t[m] / 1e9, 1)
        row['spread_' + m] = round(max(ms[m]) / t[m], 3)
    row['x2_speedup_over_fp32'] = round(t['fp32'] / t['bf16x2'], 3)
    row['x1_speedup_over_fp32'] = round(t['fp32'] / t['bf16x1'], 3)
    row['x2_is_two_term'] = 'x2' in row['kernel_bf16x2']
    row['route'] = bool(row['x2_is_two_term'] and t['bf16x2'] < t['fp32'])
    row.update(extra or {})
    return row


def bench_layers(n, rounds, dev, kinds, emit):
    for c1, c2, co, hw in SHAPES:
        x = ops.to_nhwc(torch.randn(n, c1, hw, hw, device=dev) * 1.5 + 0.3)
        x2 = ops.to_nhwc(torch.randn(n, c2, hw, hw, device=dev)) if c2 else None
        dy = ops.to_nhwc(torch.randn(n, co, hw, hw, device=dev))
        w = torch.randn(co, c1 + c2, 3, 3, device=dev) / (3 * (c1 + c2) ** 0.5)
        name = '%d+%d->%d@%d^2' % (c1, c2, co, hw)
        flops = 2.0 * 9 * (c1 + c2) * co * n * hw * hw
        if 'fwd' in kinds:
            emit(layer_row('fwd', name, n, flops, lambda m: (lambda: ops._conv_fwd_impl(x, x2, w, None, 1, 1, 0, 0.0, precision=m)), rounds))
        if 'dgrad' in kinds:
            for lo, hi in ((0, c1),) + (((c1, c1 + c2),) if c2 else ()):
                emit(layer_row('dgrad', name, n, flops * (hi - lo) / (c1 + c2),
                               lambda m: (lambda: ops._conv_dgrad_impl(dy, w, 1, 1, hw, hw, lo, hi, precision=m)), rounds, dict(slice=[lo, hi])))
        if 'wgrad' in kinds:
            emit(layer_row('wgrad', name, n, flops, lambda m: (lambda: ops._conv_wgrad_impl(x, x2, dy, w.shape, 1, 1, precision=m)), rounds))
        del x, x2, dy, w


def spread(v):
    return dict(ms=round(statistics.median(v), 3), ms_min=round(min(v), 3), ms_max=round(max(v), 3))


def _ratios(row):
    for m in MODES[1:]:
        row[m + '_over_fp32'] = round(row[m]['ms'] / row['fp32']['ms'], 4)
    return row


def _generator(dev):
    torch.manual_seed(41)
    return S.models_seg_gan.Generator(dict(arch='UNet_R_SS_v2', num_classes=3, input_channels=3, deep_supervision=False)).to(dev)


def bench_generator(n, size, reps, rounds, dev, emit):
    x = torch.randn(n, 3, size, size, device=dev)
    up = torch.randn(n, 3, size, size, device=dev) * 1e-3
    G = _generator(dev).train()

    def step(mode):
        def run():
            for p in G.parameters():
                p.grad = None
            with ops.train_precision(mode):
                G(x).backward(up)
        return run
    ms = alternate({m: step(m) for m in MODES}, reps, rounds)
    row = dict(bench='generator_fwd_bwd', bn='train_bn', n=n, size=size)
    row.update({m: spread(ms[m]) for m in MODES})
    emit(_ratios(row))


def bench_gan_step(n, size, reps, rounds, dev, emit):
    steps = {}
    gen = torch.Generator().manual_seed(7)
    inp = torch.randn(n, 3, size, size, generator=gen).to(dev)
    tgt = (torch.rand(n, 3, size, size, generator=gen) > 0.5).float().to(dev)
    for mode in MODES:
        G = _generator(dev).train()
        D = S.models_seg_gan.Discriminator(3, kernel_size=3, n_channels=64, n_blocks=8, fc_size=1024).to(dev).train()
        og = torch.optim.Adam(G.parameters(), lr=2e-5); od = torch.optim.Adam(D.parameters(), lr=2e-5)
        crit, adv, con = S.losses.BCEDiceLoss(), nn.BCEWithLogitsLoss(), nn.MSELoss()
        steps[mode] = (lambda G=G, D=D, og=og, od=od, mode=mode:
                       S.train_seg_gan.gan_step(inp, tgt, G, D, crit, adv, con, og, od, 3, precision=mode))
    ms = alternate(steps, reps, rounds)
    row = dict(bench='gan_step', n=n, size=size)
    row.update({m: spread(ms[m]) for m in MODES})
    for m in MODES:
        row['img_per_s_' + m] = round(n / row[m]['ms'] * 1e3, 2)
    emit(_ratios(row))


def bench_segment(rounds, dev, emit):
    A = S.aerial_image_segmentation_api
    G = _generator(dev).eval()
    cfg = dict(patch_size=1024, input_w=512, input_h=512, patch_overlap=0.5, num_classes=3)
    img = np.random.default_rng(5).integers(0, 256, (2048, 2048, 3), dtype=np.uint8)
    ms = alternate({m: (lambda m=m: A.segment_image(G, img, cfg, batch_size=12, precision=m)) for m in MODES}, 1, rounds)
    row = dict(bench='segment_image', image=2048, patch=1024, infer=512, batch=12)
    row.update({m: spread(ms[m]) for m in MODES})
    base = A.segment_image(G, img, cfg, batch_size=12)
    for m in MODES[1:]:
        got = A.segment_image(G, img, cfg, batch_size=12, precision=m)
        row['mask_bytes_differ_' + m] = float(np.mean([np.mean(a != b) for a, b in zip(base, got)]))
    emit(_ratios(row))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=16)
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--only', default='fwd,dgrad,wgrad,generator,gan_step,segment')
    ap.add_argument('--out', default=None, help='append the JSON lines to this file as well')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_bf16x2.py measures on the GPU'
    dev = torch.device('cuda', 0)
    kinds = set(a.only.split(','))

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if a.out:
            with open(a.out, 'a') as f:
                f.write(line + '\n')
    torch.manual_seed(0)
    if kinds & {'fwd', 'dgrad', 'wgrad'}:
        with torch.no_grad():
            bench_layers(a.n, a.rounds, dev, kinds, emit)
    if 'generator' in kinds:
        bench_generator(a.n, a.size, a.reps, a.rounds, dev, emit)
    if 'gan_step' in kinds:
        bench_gan_step(a.n, a.size, a.reps, a.rounds, dev, emit)
    if 'segment' in kinds:
        bench_segment(a.rounds, dev, emit)


if __name__ == '__main__':
    main()
