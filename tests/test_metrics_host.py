"""Quality metrics, the host side: ``rate.search_quality`` keeps its guarantees on any quality function,
``metrics.summary`` is tests/metrics_spec.py's arithmetic, and every argument error of ``metrics.compare``,
``compress(target_psnr=...)`` and ``rate.check_target`` is raised before the device is touched (these
tests run without a GPU)."""

import math
import os

import numpy as np
import pytest

import kompressor_amd as kom
from kompressor_amd import _lib, container, metrics, rate

import metrics_spec as M


def vol(dtype):
    return np.zeros((1, 5, 5, 5, 1), dtype)


def refused(tmp_path, exc, x, **kw):
    with pytest.raises(exc):
        container.compress(str(tmp_path / 'x.kmp'), x, kom.MeanPredictor(0, 3), levels=1, **kw)
    assert not os.listdir(tmp_path)


def test_exported():
    assert kom.metrics is metrics
    assert (_lib.CODER_COMPARE, _lib.COMPARE_GROUPS, _lib.COMPARE_BYTES) == (10, 1024, 64 * 1025)
    assert _lib.coder_compare() == 10 and _lib.coder_compare(True) == 10 | (1 << 8)
    assert 'target_psnr' in container.compress.__code__.co_varnames and callable(container.compare)
    assert 'kmp_code' in _lib.EXPORTED and not any('compare' in name for name in _lib.EXPORTED)


# ---- the search ----

def check_search(q, L, target):
    """The three guarantees and the probe bound for the quality table ``q``; agrees with the spec."""
    asked = []

    def quality(r):
        asked.append(r)
        return q[r]
    try:
        rung, probes = rate.search_quality(quality, L, target)
    except rate.Unreachable as e:
        assert q[L - 1] < target and q[0] < target and e.finest == q[0] and isinstance(e, ValueError)
        with pytest.raises(M.Unreachable):
            M.search_quality(lambda r: q[r], L, target)
        return None
    assert q[rung] >= target                                 # the rung meets the target
    assert rung == L - 1 or q[rung + 1] < target             # its coarser neighbour does not, or does not exist
    assert len(asked) <= 2 + math.ceil(math.log2(L)) if L > 1 else len(asked) == 1
    assert len(set(asked)) == len(asked) and probes == [(r, float(q[r])) for r in asked]
    assert (rung, probes) == M.search_quality(lambda r: q[r], L, target)
    return rung


def test_search_on_monotone_qualities():
    for L in (1, 2, 3, 4, 5, 23, 32, 128, 32768):
        q = [6.0 * (L - r) for r in range(L)]
        for target in (0.5, 6.0, 6.5, 3.0 * L, 6.0 * L, 6.0 * L + 1):
            rung = check_search(q, L, target)
            # monotone: the coarsest rung that meets the target
            want = [r for r in range(L) if q[r] >= target]
            assert rung == (max(want) if want else None)


def test_search_on_any_quality_function():
    rng = np.random.default_rng(5)
    for L in (2, 3, 7, 32, 100):
        for _ in range(40):
            q = rng.uniform(0, 100, L).tolist()
            for target in (10.0, 50.0, 90.0, 101.0):
                check_search(q, L, target)
    check_search([math.inf, 50.0, 70.0, 20.0], 4, 60)      # lossless finest rung, not monotone
    assert check_search([math.inf], 1, 1e9) == 0
    assert check_search([math.inf, -math.inf], 2, 5) == 0
    for search in (rate.search_quality, M.search_quality):  # a NaN meets nothing
        with pytest.raises(ValueError):
            search(lambda r: [math.nan, 1.0][r], 2, 5)


# ---- the host arithmetic ----

def test_summary_is_the_spec():
    rng = np.random.default_rng(1)
    x = rng.standard_normal(100).astype(np.float32)
    r = (x + rng.standard_normal(100).astype(np.float32) * np.float32(1e-3)).astype(np.float32)
    x[3] = r[3] = np.nan
    r[5] = np.inf
    for peak in (None, 2.5):
        assert metrics.summary(M.words(M.record(x, r), True), np.float32, peak) == M.compare(x, r, peak)
    for dtype in (np.uint8, np.uint16, np.int8, np.int16):
        a = rng.integers(-100, 100, 50).astype(dtype)
        b = rng.integers(-100, 100, 50).astype(dtype)
        assert metrics.summary(M.words(M.record(a, b), False), dtype) == M.compare(a, b)
    empty = metrics.compare(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32))  # answered on the host
    assert empty == M.compare(np.zeros(0, np.float32), np.zeros(0, np.float32)) and empty['psnr'] == math.inf
    assert metrics.compare(np.zeros(0, np.uint8), np.zeros(0, np.uint8), peak=3)['peak'] == 3.0
    for bad in (np.int32, np.float64, 'int64', None):
        with pytest.raises(TypeError):
            metrics.summary(np.zeros(8, np.uint64), bad)


# ---- argument errors, raised with the device untouched ----

BAD_NUMBERS = [True, False, '4', math.nan, math.inf, -math.inf, 0, 0.0, -1, -0.5, 10 ** 400, [4], b'4']


@pytest.mark.parametrize('dtype', [np.int32, np.uint32, np.float64, np.int64, np.float16, bool])
def test_compare_refuses_other_dtypes(dtype):
    with pytest.raises(TypeError):
        metrics.compare(np.zeros(4, dtype), np.zeros(4, dtype))


def test_compare_argument_errors():
    x = np.zeros((4, 4), np.float32)
    for other in (np.uint8, np.int16, np.float64):
        with pytest.raises(TypeError):
            metrics.compare(x, np.zeros((4, 4), other))
        with pytest.raises(TypeError):
            metrics.compare(np.zeros((4, 4), other), x)
    for shape in ((4, 5), (16,), (4, 4, 1), (0,)):
        with pytest.raises(ValueError):
            metrics.compare(x, np.zeros(shape, np.float32))
    for bad in BAD_NUMBERS:
        with pytest.raises(ValueError):
            metrics.compare(x, x, peak=bad)
        with pytest.raises(ValueError):
            metrics.summary(np.zeros(8, np.uint64), np.uint8, peak=bad)


@pytest.mark.parametrize('bad', BAD_NUMBERS)
def test_bad_target_psnr(bad, tmp_path):
    for x in (vol(np.float32), vol(np.uint16)):
        refused(tmp_path, ValueError, x, target_psnr=bad)


@pytest.mark.parametrize('other', [{'target_bits': 4}, {'target_ratio': 8}, {'abs_error': 1e-3}, {'rel_error': 1e-3},
                                   {'max_error': 1}])
def test_target_psnr_stands_alone(tmp_path, other):
    for x in (vol(np.float32), vol(np.uint16)):
        refused(tmp_path, ValueError, x, target_psnr=60, **other)


def test_target_psnr_modes_fit_their_dtypes(tmp_path):
    for dtype in (np.uint8, np.uint16, np.int8, np.int16):
        assert rate.check_target(np.dtype(dtype), None, None, None, target_psnr=60) == 'near'
        assert rate.check_target(np.dtype(dtype), None, None, 'near', 'planes', target_psnr=60) == 'near'
        for mode in ('abs', 'rel'):
            refused(tmp_path, ValueError, vol(dtype), target_psnr=60, target_mode=mode)
    assert rate.check_target(np.dtype(np.float32), None, None, None, target_psnr=60) == 'abs'
    assert rate.check_target(np.dtype(np.float32), None, None, 'rel', target_psnr=60.5) == 'rel'
    refused(tmp_path, ValueError, vol(np.float32), target_psnr=60, target_mode='near')
    for mode in ('psnr', '', 3, True):
        refused(tmp_path, ValueError, vol(np.float32), target_psnr=60, target_mode=mode)
    for dtype in (np.int32, np.uint32, np.float64, np.int64):
        refused(tmp_path, TypeError, vol(dtype), target_psnr=60)
        refused(tmp_path, TypeError, vol(dtype), target_psnr=60, target_mode='abs')


def test_check_target_keeps_its_callers():
    """The new keyword has a default: the positional forms of DESIGN.md §19 mean what they meant."""
    f32 = np.dtype(np.float32)
    assert rate.check_target(f32, None, None, None) is None
    assert rate.check_target(f32, 4, None, None, 'rice', 0, None, None) == 'abs'
    with pytest.raises(ValueError):
        rate.check_target(f32, None, None, 'abs')  # a mode without a target
    with pytest.raises(ValueError):
        rate.check_target(f32, 4, None, None, 'planes')  # size targets still need Rice bundles
    with pytest.raises(ValueError):
        rate.check_target(f32, 4, 8, None)
    with pytest.raises(ValueError):
        rate.check_target(f32, 4, None, None, target_psnr=60)
    with pytest.raises(ValueError):
        rate.check_target(f32, None, None, None, abs_error=1e-3, target_psnr=60)
