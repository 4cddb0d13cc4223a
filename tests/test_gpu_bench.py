"""bench.py end to end on the GPU box: the one-GPU ``--full`` line carries the contract's keys, a
plain run prints the headline alone and ``--dump-outputs`` writes what its last step computed, and
``bench.py --gpus 2`` (no external launcher) starts two ranks itself -- rehearsed with gloo, the
ranks sharing the one GPU -- and reports the world size the process group saw."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _run(args, env_extra=None, timeout=240):
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR',
                                                            'MASTER_PORT')}
    env.update(env_extra or {})
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), *args], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, r.stdout[-3000:]
    return json.loads(lines[0])


def test_bench_one_gpu_line():
    line = _run(['--full', '--steps', '3', '--warmup', '1', '--no-e2e', '--no-cpu-baseline'])
    for key in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better',
                'scaling', 'vs_baseline', 'dtype', 'data', 'config', 'roofline'):
        assert key in line, key
    assert line['n_gpus'] == 1 and line['dist']['world_size_seen'] == 1
    assert line['value'] > 0 and 0 < line['roofline']['frac'] < 1
    assert line['config']['workload'].startswith('512^3 uint16 volume as 512 tiles of 64^3')


def test_bench_plain_run_dumps_last_step(tmp_path):
    """A plain run does the timed steps only (no roofline, baseline or end-to-end leg on its line)
    and ``--dump-outputs`` writes lowres, the 7 maps and the restored volume: float32, within 64 MB,
    the restored sample equal to the same seeded draw of the seeded input (the codec is lossless)."""
    import torch
    import bench
    out = tmp_path / 'dump'
    line = _run(['--gpus', '1', '--steps', '2', '--warmup', '1', '--dump-outputs', str(out)])
    for key in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'):
        assert key in line, key
    assert line['steps'] == 2 and line['value'] > 0 and line['ms_per_step'] > 0 and line['full'] is False
    for key in ('roofline', 'cpu_baseline', 'e2e_host', 'ms_encode', 'ms_decode', 'c4'):
        assert key not in line, key
    names = ['lowres', *(f'map{i}' for i in range(7)), 'restored']
    assert sorted(os.listdir(out)) == sorted(n + '.npy' for n in names)
    arrays = [np.load(out / (n + '.npy')) for n in names]
    assert all(a.dtype == np.float32 for a in arrays)
    assert sum(os.path.getsize(out / f) for f in os.listdir(out)) <= 64 * 10**6
    # the run's inputs and its draw of elements, made again here: lowres is the even sub-grid
    # of the volume and the restored volume is the volume
    host = bench.synthetic(bench.WORKLOADS['volume'], seed=0)
    sizes = [(host.size // 8, torch.uint16)] * 8 + [(host.size, torch.uint16)]
    layout = bench.dump_layout(sizes)
    for i, want in ((0, host[:, ::2, ::2, ::2]), (8, host)):
        idx = bench.dump_index(sizes[i][0], layout[i][1], i)
        assert idx is not None and arrays[i].shape == idx.shape
        assert np.array_equal(arrays[i], want.reshape(-1)[idx].astype(np.float32)), names[i]


def test_bench_gpus2_launches_two_ranks():
    line = _run(['--full', '--gpus', '2', '--steps', '2', '--warmup', '1', '--no-e2e'], {'KMP_BENCH_BACKEND': 'gloo'})
    assert line['n_gpus'] == 2
    assert line['dist']['world_size_seen'] == 2 and line['dist']['backend'] == 'gloo'
    assert line['config']['global_batch'] == 1024
    assert line['c4']['tiles_per_rank'] == 256
    assert line['cpu_baseline'] is None  # rank 0 at N = 1 only
