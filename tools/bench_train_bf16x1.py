"""Opt-in bf16x1 training, measured.  Everything in one process on one box, the new path alternated with the
kernels the default path launches over ROUNDS rounds, HIP events, random operands; one JSON line per row:

  wgrad      per BasicBlock 3x3 shape of UNet_R_SS_v2 at N x 512^2 (N = 16): ops._conv_wgrad_impl (wgrad_k32, or whatever make_plan
             picks) against ops._conv_wgrad_bf16x1_impl (wgrad_k32_x1_kernel);
  dgrad      the same shapes: ops._conv_dgrad_impl against ops._conv_dgrad_bf16x1_impl, per input pointer of a concat conv;
  generator  forward + backward of the generator, train-mode and frozen batch norm, under train_precision 'fp32' and 'bf16x1';
  gan_step   the full G+D step in both precisions.

`route` = the new kernel was faster in this run: the rule by which a shape may stay in the bf16x1 predicates.  No speed-up is
promised: the tool states what comes out.  Usage: python tools/bench_train_bf16x1.py [--out file] [--only wgrad,dgrad,generator,gan_step]"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ssunet_gan_amd as S                                                    # noqa: E402
from ssunet_gan_amd import ops                                                # noqa: E402

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


def pair_row(kind, shape, n, flops, f32, x1, rounds, extra=None):
    if x1() is None:
        return dict(bench=kind, shape=shape, batch=n, refused=True)
    reps = max(4, int(1e12 / flops))
    ms = alternate({'fp32': f32, 'x1': x1}, reps, rounds)
    t32, tx1 = min(ms['fp32']), min(ms['x1'])
    row = dict(bench=kind, shape=shape, batch=n, fp32_kernel=label_of(f32), x1_kernel=label_of(x1), ms_fp32=round(t32, 4), ms_x1=round(tx1, 4),
               speedup=round(t32 / tx1, 3), tflops_fp32=round(flops / t32 / 1e9, 1), tflops_x1=round(flops / tx1 / 1e9, 1),
               spread_fp32=round(max(ms['fp32']) / t32, 3), spread_x1=round(max(ms['x1']) / tx1, 3), route=tx1 < t32)
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
        if 'wgrad' in kinds:
            emit(pair_row('wgrad', name, n, flops, lambda: ops._conv_wgrad_impl(x, x2, dy, w.shape, 1, 1),
                          lambda: ops._conv_wgrad_bf16x1_impl(x, x2, dy, w.shape), rounds))
        if 'dgrad' in kinds:
            for lo, hi in ((0, c1),) + (((c1, c1 + c2),) if c2 else ()):
                emit(pair_row('dgrad', name, n, flops * (hi - lo) / (c1 + c2), lambda: ops._conv_dgrad_impl(dy, w, 1, 1, hw, hw, lo, hi),
                              lambda: ops._conv_dgrad_bf16x1_impl(dy, w, hw, hw, lo, hi), rounds, dict(slice=[lo, hi])))
        del x, x2, dy, w


def spread(v):
    return dict(ms=round(statistics.median(v), 3), ms_min=round(min(v), 3), ms_max=round(max(v), 3))


def bench_generator(n, size, reps, rounds, dev, emit):
    x = torch.randn(n, 3, size, size, device=dev)
    up = torch.randn(n, 3, size, size, device=dev) * 1e-3
    for bn in ('train_bn', 'frozen_bn'):
        torch.manual_seed(41)
        G = S.models_seg_gan.Generator(dict(arch='UNet_R_SS_v2', num_classes=3, input_channels=3, deep_supervision=False)).to(dev)
        if bn == 'frozen_bn':
            S.batchnorm.freeze_batch_norm(G)
        G.train()

        def step(mode):
            def run():
                for p in G.parameters():
                    p.grad = None
                with ops.train_precision(mode):
                    G(x).backward(up)
            return run
        ms = alternate({'fp32': step('fp32'), 'bf16x1': step('bf16x1')}, reps, rounds)
        row = dict(bench='generator_fwd_bwd', bn=bn, n=n, size=size, fp32=spread(ms['fp32']), bf16x1=spread(ms['bf16x1']))
        row['bf16x1_over_fp32'] = round(row['bf16x1']['ms'] / row['fp32']['ms'], 4)
        emit(row)
        del G


def bench_gan_step(n, size, reps, rounds, dev, emit):
    steps = {}
    gen = torch.Generator().manual_seed(7)
    inp = torch.randn(n, 3, size, size, generator=gen).to(dev)
    tgt = (torch.rand(n, 3, size, size, generator=gen) > 0.5).float().to(dev)
    for mode in ('fp32', 'bf16x1'):
        torch.manual_seed(41)
        G = S.models_seg_gan.Generator(dict(arch='UNet_R_SS_v2', num_classes=3, input_channels=3, deep_supervision=False)).to(dev).train()
        D = S.models_seg_gan.Discriminator(3, kernel_size=3, n_channels=64, n_blocks=8, fc_size=1024).to(dev).train()
        og = torch.optim.Adam(G.parameters(), lr=2e-5); od = torch.optim.Adam(D.parameters(), lr=2e-5)
        crit, adv, con = S.losses.BCEDiceLoss(), nn.BCEWithLogitsLoss(), nn.MSELoss()
        steps[mode] = (lambda G=G, D=D, og=og, od=od, mode=mode:
                       S.train_seg_gan.gan_step(inp, tgt, G, D, crit, adv, con, og, od, 3, precision=mode))
    ms = alternate(steps, reps, rounds)
    row = dict(bench='gan_step', n=n, size=size, fp32=spread(ms['fp32']), bf16x1=spread(ms['bf16x1']))
    row['bf16x1_over_fp32'] = round(row['bf16x1']['ms'] / row['fp32']['ms'], 4)
    row['img_per_s_fp32'] = round(n / row['fp32']['ms'] * 1e3, 2); row['img_per_s_bf16x1'] = round(n / row['bf16x1']['ms'] * 1e3, 2)
    emit(row)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=16)
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--only', default='wgrad,dgrad,generator,gan_step')
    ap.add_argument('--out', default=None, help='append the JSON lines to this file as well')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_train_bf16x1.py measures on the GPU'
    dev = torch.device('cuda', 0)
    kinds = set(a.only.split(','))

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if a.out:
            with open(a.out, 'a') as f:
                f.write(line + '\n')
    torch.manual_seed(0)
    if kinds & {'wgrad', 'dgrad'}:
        with torch.no_grad():
            bench_layers(a.n, a.rounds, dev, kinds, emit)
    if 'generator' in kinds:
        bench_generator(a.n, a.size, a.reps, a.rounds, dev, emit)
    if 'gan_step' in kinds:
        bench_gan_step(a.n, a.size, a.reps, a.rounds, dev, emit)


if __name__ == '__main__':
    main()
