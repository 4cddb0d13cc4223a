"""bench.py --dump-outputs (CPU): what is written, in which dtype, how much, and that the draw of
elements kept from a large array is fixed."""

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import bench  # noqa: E402


def test_small_arrays_are_written_whole(tmp_path):
    a = torch.arange(2 * 3 * 5, dtype=torch.int32).reshape(2, 3, 5).to(torch.uint16)
    b = torch.tensor([0, 1, 2**32 - 1], dtype=torch.int64).to(torch.uint32)
    c = torch.linspace(-1, 1, 7, dtype=torch.float32)
    bench.dump_outputs(str(tmp_path), [('a', a), ('b', b), ('c', c)])
    assert sorted(os.listdir(tmp_path)) == ['a.npy', 'b.npy', 'c.npy']
    ra, rb, rc = (np.load(tmp_path / f) for f in ('a.npy', 'b.npy', 'c.npy'))
    assert ra.dtype == np.float32 and ra.shape == (2, 3, 5) and np.array_equal(ra.ravel(), np.arange(30))
    assert rb.dtype == np.float64 and rb.tolist() == [0.0, 1.0, float(2**32 - 1)]  # 32 bits: exact in float64
    assert rc.dtype == np.float32 and np.array_equal(rc, c.numpy())


def test_large_arrays_keep_a_fixed_draw_within_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, 'DUMP_BUDGET', 4000)
    big = (torch.arange(30000, dtype=torch.int32) % 65536).to(torch.uint16)
    small = torch.arange(10000, dtype=torch.int32).to(torch.uint8)
    for d in ('one', 'two'):
        bench.dump_outputs(str(tmp_path / d), [('big', big), ('small', small)])
    one = [np.load(tmp_path / 'one' / f) for f in ('big.npy', 'small.npy')]
    two = [np.load(tmp_path / 'two' / f) for f in ('big.npy', 'small.npy')]
    assert all(np.array_equal(x, y) for x, y in zip(one, two))
    assert sum(x.nbytes for x in one) <= 4000
    layout = bench.dump_layout([(30000, torch.uint16), (10000, torch.uint8)])
    assert [k for _, k in layout] == [750, 250]  # shares in proportion to size
    for i, (x, src) in enumerate(zip(one, (big, small))):
        idx = bench.dump_index(src.numel(), layout[i][1], i)
        assert x.ndim == 1 and 0 < x.size <= layout[i][1] and np.all(np.diff(idx) > 0)
        assert np.array_equal(x, src.numpy().astype(np.float32)[idx])


def test_steps_must_be_positive(monkeypatch):
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--steps', '0'])
    try:
        bench.parse()
    except SystemExit as e:
        assert e.code == 2
    else:
        raise AssertionError('--steps 0 was accepted')
