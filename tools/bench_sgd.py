"""Optimizer step over the stage-2 parameter sets (generator: 269 tensors, discriminator: 55), three ways:

  (a) srgan_utils.clip_gradient + torch.optim.SGD.step()   -- what an SGD config ran before optim.clip_sgd_step
  (b) optim.clip_sgd_step                                  -- one ssg_clamp_sgd_multi_f32 launch
  (c) optim.clip_adam_step                                 -- one ssg_clamp_adam_multi_f32 launch, the yardstick

HIP events around REPS back-to-back steps after a warm-up, the three paths alternated over ROUNDS rounds (median and
spread reported); device launches of one step counted in a separate torch.profiler pass, never inside a timed window.
Algorithmic bytes per element (fp32): SGD with momentum and clip reads p, g, buf and writes p, g, buf = 24; Adam with clip
reads and writes p, g, m, v = 32.  One JSON line per parameter set."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ssunet_gan_amd as S                                                    # noqa: E402

CLIP = 0.8
SGD_KW = dict(lr=1e-4, momentum=0.9, nesterov=True, weight_decay=1e-4)


def timed(fn, reps):
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def launches(fn):
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn(); torch.cuda.synchronize()
    n = sum(1 for ev in prof.events() if ev.device_type == DeviceType.CUDA and 'memcpy' not in ev.name.lower() and 'memset' not in ev.name.lower())
    return n or None                                                         # None: the profiler saw no device activity, not measured


def clones(params):
    out = [p.detach().clone().requires_grad_(True) for p in params]
    g = torch.Generator(device='cuda').manual_seed(3)
    for p in out:
        p.grad = torch.randn(p.shape, device=p.device, generator=g) * 2
    return out


def bench_set(name, params, reps, rounds, warmup):
    numel = sum(p.numel() for p in params)
    sets = [clones(params) for _ in range(3)]
    o_a = torch.optim.SGD(sets[0], **SGD_KW); o_b = torch.optim.SGD(sets[1], **SGD_KW)
    o_c = torch.optim.Adam(sets[2], lr=1e-4, weight_decay=1e-4)

    def path_a():
        S.srgan_utils.clip_gradient(o_a, CLIP); o_a.step()
    paths = (('torch_sgd', path_a, 24), ('clip_sgd_step', lambda: S.optim.clip_sgd_step(o_b, CLIP), 24),
             ('clip_adam_step', lambda: S.optim.clip_adam_step(o_c, CLIP), 32))
    for _, fn, _ in paths:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k, _, _ in paths}
    for _ in range(rounds):
        for k, fn, _ in paths:
            ms[k].append(timed(fn, reps))
    # same inputs, same result: (a) and (b) ran the same number of steps from the same values
    err = max((p.detach() - q.detach()).abs().max().item() for p, q in zip(sets[0], sets[1]))
    row = dict(set=name, tensors=len(params), numel=numel, reps=reps, rounds=rounds, max_abs_diff_torch_vs_fused=err)
    for k, fn, bpe in paths:
        med = statistics.median(ms[k])
        row[k] = dict(ms=round(med, 4), ms_min=round(min(ms[k]), 4), ms_max=round(max(ms[k]), 4), launches=launches(fn),
                      bytes_per_elem=bpe, algorithmic_GBps=round(numel * bpe / med / 1e6, 1))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_sgd.py measures on the GPU'
    dev = torch.device('cuda', 0)
    torch.manual_seed(41)
    G = S.models_seg_gan.Generator(dict(arch='UNet_R_SS_v2', num_classes=3, input_channels=3, deep_supervision=False)).to(dev)
    D = S.models_seg_gan.Discriminator(3, 3, 64, 8, 1024).to(dev)
    for name, net in (('generator', G), ('discriminator', D)):
        print(json.dumps(bench_set(name, list(net.parameters()), a.reps, a.rounds, a.warmup)), flush=True)


if __name__ == '__main__':
    main()
