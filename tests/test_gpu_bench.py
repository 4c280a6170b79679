"""bench.py run as the driver runs it (a subprocess, stdout and stderr captured), at reduced table sizes: the LAST stdout line is
the bounded contract line, every leg of a --full run is in bench_detail.json, and stderr carries no Python warning (VERDICT r4 missing #1);
a plain run runs no leg beside the headline."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_subprocess_last_stdout_line_is_the_contract_line(tmp_path):
    env = dict(os.environ, PYTHONWARNINGS='default')
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1', '--users', '2000001',
           '--items-per-domain', '1000000', '--batch', '65536', '--cpu-seconds', '0.5', '--no-config-legs', '--full']
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=str(tmp_path))
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    last = lines[-1]
    assert len(last) <= 4096, len(last)
    d = json.loads(last)
    for k in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling', 'vs_baseline', 'dtype',
              'data', 'config', 'roofline', 'cpu_baseline', 'bench_wall_s', 'detail_file'):
        assert k in d, k
    assert d['steps'] == 3 and d['warmup'] == 1 and d['n_gpus'] == 1 and d['vs_baseline'] is None
    assert abs(d['value'] - 2 * 65536 / (d['ms_per_step'] * 1e-3)) / d['value'] < 1e-6
    r = d['roofline']
    assert r['bound'] == 'hbm' and abs(r['frac'] - r['achieved'] / r['peak']) < 1e-9 and r['peak'] == 8000.0
    assert r['traffic'] is None or isinstance(r['traffic'], int)
    assert d['cpu_baseline']['kind'] == 'port' and d['cpu_baseline']['value'] > 0
    full = json.load(open(os.path.join(ROOT, d['detail_file'])))
    assert full['value'] == d['value'] and 'kernels' in full and 'e2e' in full
    bad = [l for l in p.stderr.splitlines() if 'Warning' in l or 'Traceback' in l]
    assert not bad, bad[:5]


@pytest.mark.gpu
def test_bench_plain_run_times_the_headline_steps_alone(tmp_path):
    """Without --full the run is set-up, warm-up, the timed steps and the line: the contract keys with the headline's meaning, and none
    of the legs, rooflines, checksums or CPU baselines that --full adds, neither in the line nor in the detail file."""
    detail = tmp_path / 'detail.json'
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1', '--users', '2000001',
           '--items-per-domain', '1000000', '--batch', '65536', '--detail-file', str(detail)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert p.returncode == 0, p.stderr[-3000:]
    d = json.loads([l for l in p.stdout.splitlines() if l.strip()][-1])
    assert d['metric'] == 'training interactions/sec' and d['unit'] == 'interactions/s' and d['higher_is_better'] is True and d['dtype'] == 'f32'
    assert d['steps'] == 3 and d['warmup'] == 1 and d['n_gpus'] == 1
    assert abs(d['value'] - 2 * 65536 / (d['ms_per_step'] * 1e-3)) / d['value'] < 1e-6
    assert 'two HIP streams' in d['config']['streams']
    full = json.load(open(detail))
    assert full['value'] == d['value'] and full['ms_per_step'] == d['ms_per_step']
    for k in ('roofline', 'roofline_step', 'roofline_gather', 'kernels', 'single_stream', 'state_checksum', 'state_checksum_after_all_legs',
              'overlap_phase', 'two_streams', 'mf_pointwise', 'per_positive_k4', 'synthetic_grid', 'small_batch_2048', 'fullsort', 'configs',
              'e2e', 'ingest', 'cpu_baseline', 'leg_errors'):
        assert k not in full, k
        assert k not in d, k


@pytest.mark.gpu
def test_bench_dump_outputs_are_bounded_and_repeatable(tmp_path):
    """--dump-outputs DIR: the last timed step's outputs as float32 / float64 .npy files of at most 64 MB in all, and two runs with the
    same arguments write the same numbers (the inputs are seeded, the C5 step is deterministic), so two builds compare file by file."""
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1', '--users', '2000001',
           '--items-per-domain', '1000000', '--batch', '65536', '--no-config-legs', '--no-e2e', '--no-ingest', '--no-fullsort', '--no-map',
           '--no-cpu-baseline', '--detail-file', str(tmp_path / 'detail.json')]
    dumps = []
    for run in ('a', 'b'):
        out = tmp_path / run
        p = subprocess.run(cmd + ['--dump-outputs', str(out)], capture_output=True, text=True, timeout=900, cwd=str(tmp_path))
        assert p.returncode == 0, p.stderr[-3000:]
        d = json.loads([l for l in p.stdout.splitlines() if l.strip()][-1])
        assert d['steps'] == 3 and d['ms_per_step'] > 0
        files = sorted(os.listdir(out))
        assert files and all(f.endswith('.npy') for f in files)
        assert sum(os.path.getsize(out / f) for f in files) <= 64 << 20
        arrays = {f: np.load(out / f) for f in files}
        assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
        dumps.append(arrays)
    a, b = dumps
    assert sorted(a) == sorted(b)
    for f in a:
        assert np.array_equal(a[f], b[f]), f
    for dom in ('source', 'target'):
        out6 = a[dom + '_step_out.npy']
        assert np.isfinite(out6).all() and out6[0] > 0                                   # the last step's total loss
        ids = a[dom + '_batch_ids.npy']
        assert ids.shape[1] == 3 and a[dom + '_user_rows.npy'].shape == (ids.shape[0], 128)
