"""The one-term bf16 inference conv (conv_halo_k32_bf16.hip, ops.conv2d_bf16x1) against the fp32-class kernel ops.conv2d launches for
the same tensors, per layer: the 3x3 stride-1 shapes of UNet_R_SS_v2's eval forward at 512^2, batch 9 and 12 (what segment_image
runs with and without dedupe).  HIP events, both kernels in the same process, alternated over three rounds, best round each,
random operands, bias + ReLU epilogue as in the folded BasicBlock.  One line per (shape, batch); `route` says whether the new
kernel is faster (the routing rule of DESIGN.md 3.14).  Usage: python tools/micro_x1.py [json-lines output path]"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ssunet_gan_amd import ops  # noqa: E402
from ssunet_gan_amd._lib import ACT_RELU  # noqa: E402

dev = 'cuda'
# (C1, C2, Cout, size): conv1 / conv2 of the blocks listed in the issue, plus the 64 -> 128 ... encoder conv1 shapes and the
# 192-wide column tile (three 64-channel tiles) for a per-FLOP comparison of the two tile shapes
SHAPES = [(64, 0, 64, 512), (64, 128, 64, 512), (128, 0, 128, 256), (128, 256, 128, 256), (256, 0, 256, 128), (256, 256, 256, 128),
          (384, 0, 384, 64), (384, 384, 384, 64), (512, 0, 512, 32), (512, 512, 512, 32),
          (64, 0, 128, 256), (128, 0, 256, 128), (256, 0, 384, 64), (384, 0, 512, 32), (128, 0, 192, 256)]


def label_of(fn):
    ops.PROFILE = []
    try:
        fn()
        torch.cuda.synchronize()
        return [r[0] for r in ops.PROFILE][-1]
    finally:
        ops.PROFILE = None


def event_ms(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def main():
    out = open(sys.argv[1], 'w') if len(sys.argv) > 1 else None
    torch.manual_seed(0)
    with torch.no_grad():
        for nb in (9, 12):
            for c1, c2, co, hw in SHAPES:
                x = ops.to_nhwc(torch.randn(nb, c1, hw, hw, device=dev) * 1.5 + 0.3)
                x2 = ops.to_nhwc(torch.randn(nb, c2, hw, hw, device=dev)) if c2 else None
                w = torch.randn(co, c1 + c2, 3, 3, device=dev) / (3 * (c1 + c2) ** 0.5)
                b = torch.randn(co, device=dev)
                f32 = lambda: ops.conv2d(x, w, b, 1, 1, act=ACT_RELU, x2=x2)
                x1 = lambda: ops.conv2d_bf16x1(x, w, b, act=ACT_RELU, x2=x2)
                if not ops.conv2d_bf16x1_ok(x, w, x2=x2):
                    continue
                l32, lx1 = label_of(f32), label_of(x1)
                err = (x1() - f32()).abs().max().item()
                flops = 2.0 * 9 * (c1 + c2) * co * nb * hw * hw
                n = max(4, int(2e12 / flops))
                t = {'fp32': [], 'x1': []}
                for _ in range(3):
                    for name, fn in (('fp32', f32), ('x1', x1)):
                        event_ms(fn, 2)
                        t[name].append(event_ms(fn, n))
                t32, tx1 = min(t['fp32']), min(t['x1'])
                row = {'shape': '%d+%d->%d@%d^2' % (c1, c2, co, hw), 'batch': nb, 'fp32_kernel': l32, 'x1_kernel': lx1,
                       'ms_fp32': round(t32, 4), 'ms_x1': round(tx1, 4), 'speedup': round(t32 / tx1, 3),
                       'tflops_fp32': round(flops / t32 / 1e9, 1), 'tflops_x1': round(flops / tx1 / 1e9, 1),
                       'spread_fp32': round(max(t['fp32']) / t32, 3), 'spread_x1': round(max(t['x1']) / tx1, 3),
                       'max_abs_diff': float('%.3e' % err), 'route': tx1 < t32}
                line = json.dumps(row)
                print(line, flush=True)
                if out:
                    out.write(line + '\n'); out.flush()
                del x, x2, w


if __name__ == '__main__':
    main()
