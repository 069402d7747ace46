"""wgrad32_cin_kernel (kernel id 18) on every shape of the 16 x 512^2 step that runs under it: A/B of library builds.
`python tools/micro_wgrad32.py libA.so libB.so [rounds] [--out file.jsonl]` runs each library (a file name under ssunet-gan_amd/,
loaded through SSG_LIB_PATH) in a child process of its own, alternated A B A B ... on the same box, HIP events over kernel + slab
reduce, random N(0,1) operands, and prints per shape the median and the spread (min .. max) of the per-round times of each.  The
last library counts as faster on a shape only if its max is below the first one's min (with more than two libraries there is no
verdict line).  Without library arguments: the shipped library alone.

Shapes (tools/shapes.py, profiles/r16_a_kernel_stats_bench_bs16_512.csv: 8 launches per step, all on a 2048-workgroup grid):
the 3 -> 64 image stems (the discriminator's, three times, and the generator's first conv) and the two 64-channel halves of
SPADE's 4 -> 128 gamma|beta conv, each half a channel slice of the 128-wide dout (ldd = 128).
`python tools/micro_wgrad32.py one <index>` launches shape <index> five times and exits: the program a counter pass profiles
(`rocprofv3 --kernel-trace --pmc <the counters of tools/prof_sq.sh> -- python tools/micro_wgrad32.py one 0`, with SSG_LIB_PATH
for another build; tools/sq_counters.py reads the two passes)."""
import json, os, statistics, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NB, HW = 16, 512
SHAPES = [('3->64@512', 3, 64, 64, 0), ('4->64@512 half 0 of 128', 4, 64, 128, 0), ('4->64@512 half 1 of 128', 4, 64, 128, 64)]   # Cin, Cout, dout width, offset

ONE = len(sys.argv) > 2 and sys.argv[1] == 'one'
if ONE:
    SHAPES = [SHAPES[int(sys.argv[2])]]
if ONE or (len(sys.argv) > 1 and sys.argv[1] == 'child'):
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
    for key, ci, co, wide, off in SHAPES:
        x = ops.to_nhwc(torch.randn(NB, ci, HW, HW, device='cuda'))
        dy = ops.to_nhwc(torch.randn(NB, wide, HW, HW, device='cuda'))[:, off:off + co]
        ops.PROFILE = []
        ops._conv_wgrad_impl(x, None, dy, (co, ci, 3, 3), 1, 1)
        labels = [p[0] for p in ops.PROFILE]; ops.PROFILE = None
        assert labels and labels[0].startswith('wgrad32_cin_kernel'), (key, labels)
        if ONE:
            for _ in range(4):
                ops._conv_wgrad_impl(x, None, dy, (co, ci, 3, 3), 1, 1)
            torch.cuda.synchronize()
            sys.exit(0)
        res[key] = (t(lambda: ops._conv_wgrad_impl(x, None, dy, (co, ci, 3, 3), 1, 1), 30), 4.0 * NB * HW * HW * (co + 4))
        del x, dy
    print('RESULT ' + json.dumps(res), flush=True)
    sys.exit(0)

args = sys.argv[1:]
out = None
if '--out' in args:
    i = args.index('--out'); out = args[i + 1]; del args[i:i + 2]
rounds = int(args.pop()) if args and args[-1].isdigit() else 3
libs = args or [None]
times = {lib: {} for lib in libs}
nbytes = {}
for rnd in range(rounds):
    for lib in libs:
        env = dict(os.environ)
        if lib:
            env['SSG_LIB_PATH'] = os.path.join(ROOT, 'ssunet-gan_amd', lib)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), 'child'], env=env, capture_output=True, text=True, timeout=300)
        line = [l for l in r.stdout.splitlines() if l.startswith('RESULT ')]
        if r.returncode or not line:
            print('%s: child failed (%d)\n%s' % (lib, r.returncode, r.stderr[-800:]), flush=True)
            sys.exit(1)                                     # nothing more is started on the GPU after a failed child
        for k_, (ms, nb) in json.loads(line[0][7:]).items():
            times[lib].setdefault(k_, []).append(ms); nbytes[k_] = nb
rows = []
for k_ in nbytes:
    print(k_)
    row = {'shape': k_, 'algorithmic_bytes': nbytes[k_]}
    for lib in libs:
        v = times[lib][k_]; med = statistics.median(v)
        print('  %-28s median %.4f ms (%.4f .. %.4f)  %.2f TB/s' % (lib or 'shipped', med, min(v), max(v), nbytes[k_] / med / 1e9), flush=True)
        row[lib or 'shipped'] = {'median_ms': med, 'min_ms': min(v), 'max_ms': max(v), 'tb_per_s': nbytes[k_] / med / 1e9}
    if len(libs) == 2:
        a_, b_ = times[libs[0]][k_], times[libs[1]][k_]
        row['verdict'] = 'faster' if max(b_) < min(a_) else ('slower' if min(b_) > max(a_) else 'within spread')
        print('  -> %s: %s (x%.3f)' % (libs[1], row['verdict'], statistics.median(a_) / statistics.median(b_)), flush=True)
    rows.append(row)
if out:
    with open(out, 'w') as f:
        for row in rows:
            f.write(json.dumps(row) + '\n')
