"""Opt-in bf16x1 training of the discriminator, measured.  Everything in one process on one box, the new path
alternated with the kernels the default path launches over ROUNDS rounds, HIP events, random operands; one JSON line per row:

  fwd / dgrad  per 3x3 layer of models_seg_gan.Discriminator at N x 512^2 (N = 16), the four stride-2 and the three dense stride-1
               shapes: ops._conv_fwd_impl / _conv_dgrad_impl (today's kernel) against the one-term launcher (conv_s2_k32_x1_kernel
               for stride 2, conv_halo_k32_x1_kernel for stride 1);
  wgrad        per stride-2 layer: ops._conv_wgrad_impl (today's wgrad_dma_x3 body) against ops._conv_wgrad_s2_bf16x1_impl
               (wgrad_s2_k32_x1_kernel), HIP events over kernel + slab reduce;
  disc         forward + backward of the discriminator under train_precision 'fp32' and 'bf16x1';
  gan_step     the full G+D step in the four combinations of precision x d_precision;
  gan_step_s2  the full G+D step under d_precision='bf16x1' with d_wgrad_s2 off / on, generator 'fp32' and 'bf16x1'.

`route` = the new kernel was faster in this run by more than the run-to-run spread of the two rows: the rule by which a shape may
stay in the bf16x1 predicates; `keep` = the stricter form of DESIGN 3.14 / 3.16 / 3.18, the new kernel's WORST round beats the old
kernel's BEST round.  No speed-up is promised: the tool states what comes out.
Usage: python tools/bench_disc_bf16x1.py [--out file] [--only fwd,dgrad,wgrad,disc,gan_step,gan_step_s2]"""
import argparse
import json
import os
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ssunet_gan_amd as S                                                    # noqa: E402
from ssunet_gan_amd import ops                                                # noqa: E402
from bench_train_bf16x1 import alternate, label_of, spread                    # noqa: E402

# (Cin, Cout, stride, input size at 512^2): the discriminator's 3x3 layers behind the 3 -> 64 stem
SHAPES = [(64, 64, 2, 512), (64, 128, 1, 256), (128, 128, 2, 256), (128, 256, 1, 128), (256, 256, 2, 128), (256, 512, 1, 64), (512, 512, 2, 64)]


def labels_of(fn):
    ops.PROFILE = []
    try:
        fn()
        torch.cuda.synchronize()
        return [r[0] for r in ops.PROFILE]
    finally:
        ops.PROFILE = None


def pair_row(kind, shape, n, flops, f32, x1, rounds):
    if x1() is None:
        return dict(bench=kind, shape=shape, batch=n, refused=True)
    reps = max(4, int(1e12 / flops))
    ms = alternate({'fp32': f32, 'x1': x1}, reps, rounds)
    t32, tx1 = min(ms['fp32']), min(ms['x1'])
    s32, sx1 = max(ms['fp32']) / t32, max(ms['x1']) / tx1
    return dict(bench=kind, shape=shape, batch=n, fp32_kernel=labels_of(f32), x1_kernel=labels_of(x1), ms_fp32=round(t32, 4), ms_x1=round(tx1, 4),
                speedup=round(t32 / tx1, 3), tflops_fp32=round(flops / t32 / 1e9, 1), tflops_x1=round(flops / tx1 / 1e9, 1),
                spread_fp32=round(s32, 3), spread_x1=round(sx1, 3), route=bool(t32 / tx1 > max(s32, sx1)),
                keep=bool(max(ms['x1']) < t32))


def bench_layers(n, rounds, dev, kinds, emit):
    for ci, co, s, hw in SHAPES:
        oh = (hw - 1) // s + 1
        x = ops.to_nhwc(torch.randn(n, ci, hw, hw, device=dev) * 1.5 + 0.3)
        dy = ops.to_nhwc(torch.randn(n, co, oh, oh, device=dev))
        w = torch.randn(co, ci, 3, 3, device=dev) / (3 * ci ** 0.5)
        b = torch.randn(co, device=dev)
        name = '%d->%d s%d @%d^2' % (ci, co, s, hw)
        flops = 2.0 * 9 * ci * co * n * oh * oh
        if 'fwd' in kinds:
            new = (lambda: ops._conv_s2_bf16x1_impl(x, w, b, 0, 0.0)) if s == 2 else (lambda: ops._conv_bf16x1_impl(x, w, b, 0, 0.0))
            emit(pair_row('fwd', name, n, flops, lambda: ops._conv_fwd_impl(x, None, w, b, s, 1, 0, 0.0), new, rounds))
        if 'dgrad' in kinds:
            new = (lambda: ops._conv_dgrad_s2_bf16x1_impl(dy, w, hw, hw, 0, ci)) if s == 2 else (lambda: ops._conv_dgrad_bf16x1_impl(dy, w, hw, hw, 0, ci))
            emit(pair_row('dgrad', name, n, flops, lambda: ops._conv_dgrad_impl(dy, w, s, 1, hw, hw, 0, ci), new, rounds))
        if 'wgrad' in kinds and s == 2:
            emit(pair_row('wgrad', name, n, flops, lambda: ops._conv_wgrad_impl(x, None, dy, (co, ci, 3, 3), 2, 1),
                          lambda: ops._conv_wgrad_s2_bf16x1_impl(x, dy, (co, ci, 3, 3)), rounds))
        del x, dy, w


def bench_disc(n, size, reps, rounds, dev, emit):
    torch.manual_seed(41)
    D = S.models_seg_gan.Discriminator(3, kernel_size=3, n_channels=64, n_blocks=8, fc_size=1024).to(dev).train()
    x = torch.randn(n, 3, size, size, device=dev).requires_grad_(True)

    def step(mode):
        def run():
            for p in D.parameters():
                p.grad = None
            x.grad = None
            with ops.train_precision(mode):
                D(x).sum().backward()
        return run
    ms = alternate({'fp32': step('fp32'), 'bf16x1': step('bf16x1')}, reps, rounds)
    row = dict(bench='disc_fwd_bwd', n=n, size=size, fp32=spread(ms['fp32']), bf16x1=spread(ms['bf16x1']))
    row['bf16x1_over_fp32'] = round(row['bf16x1']['ms'] / row['fp32']['ms'], 4)
    emit(row)


def bench_gan_step(n, size, reps, rounds, dev, emit):
    steps = {}
    gen = torch.Generator().manual_seed(7)
    inp = torch.randn(n, 3, size, size, generator=gen).to(dev)
    tgt = (torch.rand(n, 3, size, size, generator=gen) > 0.5).float().to(dev)
    for mode in ('fp32', 'bf16x1'):
        for dmode in ('fp32', 'bf16x1'):
            torch.manual_seed(41)
            G = S.models_seg_gan.Generator(dict(arch='UNet_R_SS_v2', num_classes=3, input_channels=3, deep_supervision=False)).to(dev).train()
            D = S.models_seg_gan.Discriminator(3, kernel_size=3, n_channels=64, n_blocks=8, fc_size=1024).to(dev).train()
            og = torch.optim.Adam(G.parameters(), lr=2e-5); od = torch.optim.Adam(D.parameters(), lr=2e-5)
            crit, adv, con = S.losses.BCEDiceLoss(), nn.BCEWithLogitsLoss(), nn.MSELoss()
            steps['g_%s/d_%s' % (mode, dmode)] = (lambda G=G, D=D, og=og, od=od, mode=mode, dmode=dmode: S.train_seg_gan.gan_step(
                inp, tgt, G, D, crit, adv, con, og, od, 3, precision=mode, d_precision=dmode))
    ms = alternate(steps, reps, rounds)
    row = dict(bench='gan_step', n=n, size=size)
    for k, v in ms.items():
        row[k] = spread(v)
    base = row['g_fp32/d_fp32']['ms']
    for k in ms:
        row[k]['over_default'] = round(row[k]['ms'] / base, 4)
        row[k]['img_per_s'] = round(n / row[k]['ms'] * 1e3, 2)
    emit(row)


def bench_gan_step_s2(n, size, reps, rounds, dev, emit):
    steps = {}
    gen = torch.Generator().manual_seed(7)
    inp = torch.randn(n, 3, size, size, generator=gen).to(dev)
    tgt = (torch.rand(n, 3, size, size, generator=gen) > 0.5).float().to(dev)
    for mode in ('fp32', 'bf16x1'):
        for s2 in ('fp32', 'bf16x1'):
            torch.manual_seed(41)
            G = S.models_seg_gan.Generator(dict(arch='UNet_R_SS_v2', num_classes=3, input_channels=3, deep_supervision=False)).to(dev).train()
            D = S.models_seg_gan.Discriminator(3, kernel_size=3, n_channels=64, n_blocks=8, fc_size=1024).to(dev).train()
            og = torch.optim.Adam(G.parameters(), lr=2e-5); od = torch.optim.Adam(D.parameters(), lr=2e-5)
            crit, adv, con = S.losses.BCEDiceLoss(), nn.BCEWithLogitsLoss(), nn.MSELoss()
            steps['g_%s/d_bf16x1/s2_%s' % (mode, s2)] = (lambda G=G, D=D, og=og, od=od, mode=mode, s2=s2: S.train_seg_gan.gan_step(
                inp, tgt, G, D, crit, adv, con, og, od, 3, precision=mode, d_precision='bf16x1', d_wgrad_s2=s2))
    ms = alternate(steps, reps, rounds)
    row = dict(bench='gan_step_s2', n=n, size=size)
    for k, v in ms.items():
        row[k] = spread(v)
        row[k]['rounds_ms'] = [round(t, 3) for t in v]
        row[k]['img_per_s'] = round(n / row[k]['ms'] * 1e3, 2)
    for mode in ('fp32', 'bf16x1'):
        off, on = 'g_%s/d_bf16x1/s2_fp32' % mode, 'g_%s/d_bf16x1/s2_bf16x1' % mode
        row[on]['over_off'] = round(row[on]['ms'] / row[off]['ms'], 4)
        row[on]['keep'] = bool(max(ms[on]) < min(ms[off]))
    emit(row)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=16)
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--only', default='fwd,dgrad,wgrad,disc,gan_step,gan_step_s2')
    ap.add_argument('--out', default=None, help='append the JSON lines to this file as well')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_disc_bf16x1.py measures on the GPU'
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
    if 'disc' in kinds:
        bench_disc(a.n, a.size, a.reps, a.rounds, dev, emit)
    if 'gan_step' in kinds:
        bench_gan_step(a.n, a.size, a.reps, a.rounds, dev, emit)
    if 'gan_step_s2' in kinds:
        bench_gan_step_s2(a.n, a.size, a.reps, a.rounds, dev, emit)


if __name__ == '__main__':
    main()
