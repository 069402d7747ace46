"""thin4_cout (wide input, <= 8 output channels, 3x3) and the weight gradient of the same layers at 16 images: A/B of library builds.
`python tools/micro_thin_cout.py libA.so libB.so [rounds]` runs each library (a file name under ssunet-gan_amd/, loaded through
SSG_LIB_PATH) in a child process of its own, alternated A B A B ... on the same box, and prints per shape the median and the
spread (min .. max) of the per-round times of each.  Without arguments: the shipped library alone."""
import json, os, statistics, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FWD = [(64, 3, 512), (128, 4, 512), (256, 8, 256), (128, 3, 256), (256, 3, 128), (128, 8, 128)]
WGRAD = [(64, 3, 512), (128, 3, 256)]
if len(sys.argv) > 1 and sys.argv[1] == 'child':
    sys.path.insert(0, ROOT)
    import torch
    import ssunet_gan_amd as S
    from ssunet_gan_amd import ops
    from ssunet_gan_amd._lib import ACT_NONE
    torch.manual_seed(0)

    def t(fn):
        for _ in range(3): fn()
        torch.cuda.synchronize()
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20): fn()
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) / 20
    res = {}
    for (ci, co, hw) in FWD:
        x = ops.to_nhwc(torch.randn(16, ci, hw, hw, device='cuda')); w = torch.randn(co, ci, 3, 3, device='cuda')
        res['fwd %d->%d@%d' % (ci, co, hw)] = (t(lambda: ops._conv_fwd_impl(x, None, w, None, 1, 1, ACT_NONE, 0.0)), 16 * hw * hw * 4 * (ci + 4))
        del x
    for (ci, co, hw) in WGRAD:
        x = ops.to_nhwc(torch.randn(16, ci, hw, hw, device='cuda')); dy = ops.to_nhwc(torch.randn(16, co, hw, hw, device='cuda'))
        res['wgrad %d->%d@%d' % (ci, co, hw)] = (t(lambda: ops._conv_wgrad_impl(x, None, dy, (co, ci, 3, 3), 1, 1)), 16 * hw * hw * 4 * (ci + 4))
        del x, dy
    print('RESULT ' + json.dumps(res), flush=True)
    sys.exit(0)
args = sys.argv[1:]
rounds = int(args.pop()) if args and args[-1].isdigit() else 3
libs = args or [None]
times = {lib: {} for lib in libs}
nbytes = {}
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
        for k, (ms, by) in json.loads(line[0][7:]).items():
            times[lib].setdefault(k, []).append(ms); nbytes[k] = by
for k in nbytes:
    print(k)
    for lib in libs:
        v = times[lib][k]; med = statistics.median(v)
        print('  %-28s median %.3f ms (%.3f .. %.3f)  %.2f TB/s' % (lib or 'shipped', med, min(v), max(v), nbytes[k] / med / 1e9), flush=True)
