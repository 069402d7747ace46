"""Split (bf16x3) LDS-DMA convolution (kernel ids 50 / 51) on every shape of the 16 x 512^2 step that uses it: A/B of library builds.
`python tools/micro_conv_dma.py libA.so libB.so [rounds] [--out file.jsonl]` runs each library (a file name under ssunet-gan_amd/,
loaded through SSG_LIB_PATH) in a child process of its own, alternated A B A B ... on the same box, HIP events, random N(0,1)
operands (constants flatter the bf16 pipe: DESIGN.md 3.9), and prints per shape the median and the spread (min .. max) of the
per-round times of each.  The last library counts as faster on a shape only if its max is below the first one's min.  Without
library arguments: the shipped library alone.  Shapes: the 'fwd' rows of tests/test_conv_plan.py's step labelled
conv_igemm_dma_x3_kernel<...>, as (Cin, H = W, Cout, k, stride) at 16 images (the 1x1 input gradients of the step are 1x1 forwards
of the transposed pack: the same launches); MICRO_CONV_SHAPES="Cin,HW,Cout,k,stride;..." times other shapes of the label instead
(with more than two libraries there is no verdict line)."""
import json, os, statistics, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(64, 512, 64, 3, 2), (128, 256, 128, 3, 2), (256, 128, 256, 3, 2), (512, 64, 512, 3, 2),
          (192, 512, 64, 1, 1), (128, 256, 256, 1, 1), (384, 256, 128, 1, 1), (128, 256, 128, 1, 1), (128, 256, 64, 1, 1),
          (256, 128, 256, 1, 1), (512, 128, 256, 1, 1), (128, 128, 256, 1, 1), (256, 128, 128, 1, 1),
          (384, 64, 384, 1, 1), (768, 64, 384, 1, 1), (256, 64, 384, 1, 1), (384, 64, 256, 1, 1),
          (512, 32, 512, 1, 1), (512, 32, 384, 1, 1), (384, 32, 512, 1, 1), (1024, 32, 512, 1, 1),
          (768, 16, 512, 1, 1), (512, 16, 768, 1, 1)]
NB = 16
if os.environ.get('MICRO_CONV_SHAPES'):                  # other shapes of the family: "Cin,HW,Cout,k,stride;..."
    SHAPES = [tuple(int(v) for v in s.split(',')) for s in os.environ['MICRO_CONV_SHAPES'].split(';')]


def key(s):
    return '%d->%d@%d k%d s%d' % (s[0], s[2], s[1], s[3], s[4])


if len(sys.argv) > 1 and sys.argv[1] == 'child':
    sys.path.insert(0, ROOT)
    import torch
    import ssunet_gan_amd as S                           # noqa: F401
    from ssunet_gan_amd import ops
    torch.manual_seed(0)

    def t(fn, reps):
        for _ in range(3): fn()
        torch.cuda.synchronize()
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps): fn()
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps
    res = {}
    for s in SHAPES:
        ci, hw, co, k, st = s
        oh = (hw + 2 * (k // 2) - k) // st + 1
        x = ops.to_nhwc(torch.randn(NB, ci, hw, hw, device='cuda')); w = torch.randn(co, ci, k, k, device='cuda') / (k * ci ** 0.5)
        out = ops.new_nhwc(NB, co, oh, oh, x.device)
        fn = lambda: ops._conv_fwd_impl(x, None, w, None, st, k // 2, 0, 0.0, out=out)
        ops.PROFILE = []
        fn()
        labels = [p[0] for p in ops.PROFILE]; ops.PROFILE = None
        assert labels and labels[0].startswith('conv_igemm_dma_x3_kernel<'), (key(s), labels)
        res[key(s)] = (t(fn, 20), 2.0 * k * k * ci * co * NB * oh * oh)
        del x, w, out
    print('RESULT ' + json.dumps(res), flush=True)
    sys.exit(0)

args = sys.argv[1:]
out = None
if '--out' in args:
    i = args.index('--out'); out = args[i + 1]; del args[i:i + 2]
rounds = int(args.pop()) if args and args[-1].isdigit() else 3
libs = args or [None]
times = {lib: {} for lib in libs}
flops = {}
for rnd in range(rounds):
    for lib in libs:
        env = dict(os.environ)
        if lib:
            env['SSG_LIB_PATH'] = os.path.join(ROOT, 'ssunet-gan_amd', lib)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), 'child'], env=env, capture_output=True, text=True)
        line = [l for l in r.stdout.splitlines() if l.startswith('RESULT ')]
        if r.returncode or not line:
            print('%s: child failed (%d)\n%s' % (lib, r.returncode, r.stderr[-800:]), flush=True)
            sys.exit(1)                                     # nothing more is started on the GPU after a failed child
        for k_, (ms, fl) in json.loads(line[0][7:]).items():
            times[lib].setdefault(k_, []).append(ms); flops[k_] = fl
rows = []
for k_ in flops:
    print(k_)
    row = {'shape': k_, 'flop': flops[k_]}
    for lib in libs:
        v = times[lib][k_]; med = statistics.median(v)
        print('  %-28s median %.4f ms (%.4f .. %.4f)  %.1f TFLOP/s' % (lib or 'shipped', med, min(v), max(v), flops[k_] / med / 1e9), flush=True)
        row[lib or 'shipped'] = {'median_ms': med, 'min_ms': min(v), 'max_ms': max(v), 'tflops': flops[k_] / med / 1e9}
    if len(libs) == 2:
        a_, b_ = times[libs[0]][k_], times[libs[1]][k_]
        row['verdict'] = 'faster' if max(b_) < min(a_) else ('slower' if min(b_) > max(a_) else 'within spread')
        print('  -> %s: %s (x%.3f)' % (libs[1], row['verdict'], statistics.median(a_) / statistics.median(b_)), flush=True)
    rows.append(row)
if out:
    with open(out, 'w') as f:
        for row in rows:
            f.write(json.dumps(row) + '\n')
