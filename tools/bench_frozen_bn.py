"""Frozen batch norm, measured.  Two comparisons, one JSON line each:

  generator   forward + backward of Generator(UNet_R_SS_v2) at N x 3 x 512 x 512 (N = 16), batch norms frozen
              (batchnorm.freeze_batch_norm: every BasicBlock is one blocks._FrozenBasicBlockFn, no batch-norm pass in either
              direction) against train-mode batch norm on the same build (blocks._BasicBlockFn, the kernels as they were).
              The two are alternated in one process over ROUNDS rounds; HIP events around REPS synchronised iterations, after a warm-up.
  kernel      ssg_bn_frozen_bwd_f32 in its "activation backward + bias gradient" form (x = mean = scale = NULL) against the pair it
              replaces, ssg_act_bwd_f32 followed by ssg_channel_sum_f32, on the same tensors; and its eval-BN form (dx = g scale, both
              sums) on its own.  Algorithmic bytes are computed here from the shapes: one pass = 4 P C bytes; the pair reads y, dy,
              writes dx, reads dx again (4 passes), the fused form reads y, dy, writes dx (3); the eval-BN form reads x, dy, writes dx (3).
              Reported as GB/s of algorithmic bytes and as a share of the copy ceiling DESIGN.md quotes (6.3 TB/s achievable), next to
              ssg_tool_copy_f32 on the same tensors in the same run.

No speed-up is promised: the tool states what comes out."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ssunet_gan_amd as S                                                    # noqa: E402
from ssunet_gan_amd._lib import ACT_RELU, call, ptr, stream_ptr              # noqa: E402

COPY_CEILING_GBPS = 6300.0


def timed(fn, reps):
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def spread(v):
    return dict(ms=round(statistics.median(v), 4), ms_min=round(min(v), 4), ms_max=round(max(v), 4))


def bench_generator(n, size, reps, rounds, warmup, dev):
    models = {}
    for name in ('train_bn', 'frozen_bn'):
        torch.manual_seed(41)
        G = S.models_seg_gan.Generator(dict(arch='UNet_R_SS_v2', num_classes=3, input_channels=3, deep_supervision=False)).to(dev)
        if name == 'frozen_bn':
            S.batchnorm.freeze_batch_norm(G)
        models[name] = G.train()
    x = torch.randn(n, 3, size, size, device=dev)
    up = torch.randn(n, 3, size, size, device=dev) * 1e-3

    def step(G):
        def run():
            for p in G.parameters():
                p.grad = None
            G(x).backward(up)
        return run
    steps = {k: step(G) for k, G in models.items()}
    for fn in steps.values():
        for _ in range(warmup):
            fn()
    ms = {k: [] for k in steps}
    for _ in range(rounds):
        for k, fn in steps.items():
            ms[k].append(timed(fn, reps))
    row = dict(bench='generator_fwd_bwd', n=n, size=size, reps=reps, rounds=rounds)
    for k in steps:
        row[k] = spread(ms[k])
    row['frozen_over_train'] = round(row['frozen_bn']['ms'] / row['train_bn']['ms'], 4)
    return row


def bench_kernel(n, size, c, reps, rounds, warmup, dev):
    p = n * size * size
    ops = S.ops
    y = torch.randn(p * c, device=dev).view(n, size, size, c).permute(0, 3, 1, 2)
    dy = torch.randn(p * c, device=dev).view(n, size, size, c).permute(0, 3, 1, 2)
    dx = ops.new_nhwc(n, c, size, size, dev)
    out = torch.empty(c, device=dev)
    sums = torch.empty(2 * c, dtype=torch.float64, device=dev)
    ws = ops._ws(call('ssg_bn_workspace_bytes', p, c), dev)
    mean = torch.randn(c, device=dev); invstd = torch.rand(c, device=dev) + 0.5; scale = torch.randn(c, device=dev); shift = torch.randn(c, device=dev)

    def pair():
        call('ssg_act_bwd_f32', ptr(y), c, ptr(dy), c, p, c, ACT_RELU, 0.0, ptr(dx), c, stream_ptr())
        call('ssg_channel_sum_f32', ptr(dx), p, c, c, ptr(out), ptr(ws), stream_ptr())

    def fused():
        call('ssg_bn_frozen_bwd_f32', None, ptr(y), ptr(dy), p, c, 0, c, c, None, None, None, None, ACT_RELU, 0.0, ptr(dx), c, None, 0,
             ptr(sums), ptr(ws), stream_ptr())

    def eval_bn():                                            # x plays y's part: mask recomputed from x, dx = g scale, both sums
        call('ssg_bn_frozen_bwd_f32', ptr(y), None, ptr(dy), p, c, c, 0, c, ptr(mean), ptr(invstd), ptr(scale), ptr(shift), ACT_RELU, 0.0,
             ptr(dx), c, None, 0, ptr(sums), ptr(ws), stream_ptr())

    def copy():
        call('ssg_tool_copy_f32', ptr(y), ptr(dx), p * c, stream_ptr())
    one = 4.0 * p * c
    paths = (('act_bwd_plus_channel_sum', pair, 4 * one), ('frozen_bwd_bias_form', fused, 3 * one), ('frozen_bwd_eval_bn_form', eval_bn, 3 * one),
             ('copy', copy, 2 * one))
    for _, fn, _ in paths:
        for _ in range(warmup):
            fn()
    ms = {k: [] for k, _, _ in paths}
    for _ in range(rounds):
        for k, fn, _ in paths:
            ms[k].append(timed(fn, reps))
    row = dict(bench='kernel', P=p, C=c, reps=reps, rounds=rounds, copy_ceiling_GBps=COPY_CEILING_GBPS)
    for k, _, nbytes in paths:
        r = spread(ms[k])
        r['algorithmic_bytes'] = int(nbytes)
        r['algorithmic_GBps'] = round(nbytes / r['ms'] / 1e6, 1)
        r['share_of_copy_ceiling'] = round(r['algorithmic_GBps'] / COPY_CEILING_GBPS, 3)
        row[k] = r
    row['fused_over_pair_time'] = round(row['frozen_bwd_bias_form']['ms'] / row['act_bwd_plus_channel_sum']['ms'], 4)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=16)
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--kernel-reps', type=int, default=20)
    ap.add_argument('--out', default=None, help='append the JSON lines to this file as well')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_frozen_bn.py measures on the GPU'
    dev = torch.device('cuda', 0)
    rows = [bench_kernel(a.n, s, c, a.kernel_reps, a.rounds, a.warmup, dev) for s, c in ((a.size, 64), (a.size // 4, 256))]
    rows.append(bench_generator(a.n, a.size, a.reps, a.rounds, a.warmup, dev))
    for row in rows:
        line = json.dumps(row)
        print(line, flush=True)
        if a.out:
            with open(a.out, 'a') as f:
                f.write(line + '\n')


if __name__ == '__main__':
    main()
