"""CPU rehearsal of `bench.py --gpus N`: the parent must start N ranks itself (torch.distributed.run as a child process),
the ranks must form a world of N, and a WORLD_SIZE / --gpus mismatch must fail loudly instead of silently measuring one GPU
(bench.py:111).  --launch-check runs the launcher, rendezvous and rank bookkeeping without the GPU step."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT


def _run(args, env_extra, timeout=170):
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    env.update(env_extra)
    return subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + args, env=env, capture_output=True, text=True, timeout=timeout)


@pytest.mark.timeout(180)
def test_bench_gpus2_starts_two_ranks_over_gloo():
    r = _run(['--gpus', '2', '--launch-check'], {'SSG_DIST_BACKEND': 'gloo'})
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, r.stdout                       # rank 0 only
    line = json.loads(lines[0])
    assert line['n_gpus'] == 2 and line['backend'] == 'gloo' and line['rank_sum'] == 3.0


@pytest.mark.timeout(240)
def test_bench_gpus8_starts_eight_ranks_over_gloo():
    """The N = 8 shape of the driver's scaling run (BASELINE config 3), rehearsed on CPU: eight ranks, one process group,
    one JSON line from rank 0, a destroyed group on every rank (no 'destroy_process_group() was not called' warning)."""
    r = _run(['--gpus', '8', '--launch-check'], {'SSG_DIST_BACKEND': 'gloo', 'OMP_NUM_THREADS': '1'}, timeout=230)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line['n_gpus'] == 8 and line['backend'] == 'gloo' and line['rank_sum'] == 36.0
    assert 'destroy_process_group() was not called' not in r.stderr


@pytest.mark.timeout(60)
def test_bench_refuses_to_self_launch_under_a_profiler_preload():
    """under rocprofv3 the parent has already initialised the GPU; starting the launcher from it is the forbidden
    exec hop.  bench.py must refuse (exit 2) instead."""
    r = _run(['--gpus', '2', '--launch-check'], {'SSG_DIST_BACKEND': 'gloo', 'ROCPROF_KERNEL_TRACE': '1'}      )
    assert r.returncode == 2 and 'refusing to self-launch' in r.stderr


@pytest.mark.timeout(60)
def test_bench_refuses_world_size_mismatch():
    r = _run(['--gpus', '2', '--launch-check'], {'WORLD_SIZE': '1', 'RANK': '0'})
    assert r.returncode == 2 and 'WORLD_SIZE=1 but --gpus 2' in r.stderr


def test_pmc_traffic_rows_cover_the_mfma_kernels_of_the_tracked_trace():
    """bench.py reads roofline.traffic from the newest tracked PMC summary by kernel symbol.  Every MFMA conv / weight-gradient
    kernel that the newest tracked kernel trace of the bench shows must have a row there: a renamed or new kernel fails
    here instead of silently printing a stale (or no) number."""
    import csv
    import glob
    sys.path.insert(0, ROOT)
    import bench
    src, table = bench.pmc_traffic_table()
    assert src and table, 'no profiles/rNN_*pmc_hbm_traffic_per_kernel.csv'
    traces = sorted(glob.glob(os.path.join(ROOT, 'profiles', 'r[0-9][0-9]_*kernel_stats_bench_bs16_512.csv')))     # traces of bench.py itself
    assert traces
    assert os.path.basename(traces[-1])[:3] == os.path.basename(src)[:3], 'PMC summary %s is older than the kernel trace %s' % (src, traces[-1])
    names = [bench._norm_symbol(r['Name']) for r in csv.DictReader(open(traces[-1]))]
    mfma = [n for n in names if n.startswith(('conv_igemm', 'wgrad_halo', 'wgrad_dma', 'wgrad_kernel', 'gemm_bf16'))]
    assert mfma
    missing = [n for n in mfma if n not in table]
    assert not missing, 'no PMC traffic row in %s for %s' % (src, missing)


@pytest.mark.timeout(60)
def test_bench_refuses_zero_steps():
    r = _run(['--steps', '0'], {})
    assert r.returncode != 0 and '--steps must be >= 1' in r.stderr


def test_dump_outputs_of_the_bench_models_is_a_fixed_float32_sample_under_64_mb(tmp_path):
    """--dump-outputs on the bench's own G and D: float32 .npy files, at most 64 MB in all, the same parameter sample in
    every run (two builds are compared output for output)."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    import ssunet_gan_amd as S
    torch.manual_seed(41)
    G = S.models_seg_gan.Generator(dict(arch='UNet_R_SS_v2', num_classes=3, input_channels=3, deep_supervision=False))
    D = S.models_seg_gan.Discriminator(3, kernel_size=3, n_channels=64, n_blocks=8, fc_size=1024)
    out = tuple(torch.tensor(0.5 + i) for i in range(6))
    sizes = [bench.dump_outputs(str(tmp_path / d), out, (('G', G), ('D', D))) for d in ('a', 'b')]
    names = sorted(os.listdir(str(tmp_path / 'a')))
    assert names == sorted(n + '.npy' for n in bench.DUMP_NAMES + ('G_params_sample', 'G_buffers', 'D_params_sample', 'D_buffers'))
    total = 0
    for n in names:
        a, b = np.load(str(tmp_path / 'a' / n)), np.load(str(tmp_path / 'b' / n))
        assert a.dtype == np.float32 and np.array_equal(a, b), n
        total += os.path.getsize(str(tmp_path / 'a' / n))
    assert sizes[0] == sizes[1] and total <= 64 << 20
    assert np.load(str(tmp_path / 'a' / 'adv_d.npy')) == np.float32(5.5)
    assert np.load(str(tmp_path / 'a' / 'G_params_sample.npy')).size == bench.DUMP_SAMPLE


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_plain_bench_times_its_steps_and_dumps_the_last_one(tmp_path):
    """A plain run (no --full): exactly --steps timed steps, ms_per_step in the line, none of the --full legs, and the outputs of
    the last timed step under --dump-outputs."""
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    d = str(tmp_path / 'out')
    r = _run(['--steps', '3', '--warmup', '1', '--batch', '2', '--size', '64', '--dump-outputs', d], {}, timeout=280)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line['steps'] == 3 and line['full'] is False and 'timed 3 steps' in r.stderr
    assert line['unit'] == 'images/sec' and line['higher_is_better'] is True and line['dtype'] == 'f32'
    assert line['ms_per_step'] > 0 and abs(line['value'] * line['ms_per_step'] / 1e3 - 2) < 0.01 * 2
    for k in ('roofline', 'fp32_mfma_reference', 'measured_ceilings', 'cpu_baseline', 'config4_b4_bf16', 'config5_infer'):
        assert k not in line, k
    got = {n: np.load(os.path.join(d, n + '.npy')) for n in ('loss', 'iou', 'dice', 'G_params_sample', 'D_params_sample')}
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in got.values())
    assert abs(float(got['loss']) - line['loss']) < 1e-6 and abs(float(got['dice']) - line['dice']) < 1e-6
