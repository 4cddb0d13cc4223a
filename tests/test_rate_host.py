"""Rate control, the host side: every argument error of ``compress(target_*)`` and of
``compressed_size`` is raised before the device is touched (these tests run without a GPU), and the
ladders' end points follow tests/rate_spec.py."""

import math
import os

import numpy as np
import pytest

import kompressor_amd as kom
from kompressor_amd import container, rate

import rate_spec as R

FLT_MAX = float(np.finfo(np.float32).max)
SUBNORMAL = float(np.float32(1e-45))


def vol(dtype):
    return np.zeros((1, 5, 5, 5, 1), dtype)


def refused(tmp_path, exc, x, **kw):
    with pytest.raises(exc):
        container.compress(str(tmp_path / 'x.kmp'), x, kom.MeanPredictor(0, 3), levels=1, **kw)
    assert not os.listdir(tmp_path)


def test_exported():
    assert kom.rate is rate
    assert 'target_bits' in container.compress.__code__.co_varnames
    assert callable(container.compressed_size) and callable(kom.packing.bundle_size) and callable(kom.packing.encoded_size)


BAD_TARGETS = [True, False, '4', math.nan, math.inf, -math.inf, 0, 0.0, -1, -0.5, 10 ** 400, [4], b'4']


@pytest.mark.parametrize('bad', BAD_TARGETS)
def test_bad_target(bad, tmp_path):
    for x in (vol(np.float32), vol(np.uint16)):
        refused(tmp_path, ValueError, x, target_bits=bad)
        refused(tmp_path, ValueError, x, target_ratio=bad)


def test_one_target_only(tmp_path):
    refused(tmp_path, ValueError, vol(np.float32), target_bits=4, target_ratio=8)
    refused(tmp_path, ValueError, vol(np.float32), target_mode='abs')  # a mode without a target
    refused(tmp_path, ValueError, vol(np.uint8), target_mode='near')


@pytest.mark.parametrize('bound', [{'abs_error': 1e-3}, {'rel_error': 1e-3}, {'max_error': 1}])
@pytest.mark.parametrize('target', [{'target_bits': 4}, {'target_ratio': 8}])
def test_targets_exclude_the_bounds(tmp_path, bound, target):
    for x in (vol(np.float32), vol(np.uint16)):
        refused(tmp_path, ValueError, x, **bound, **target)


def test_targets_need_rice(tmp_path):
    refused(tmp_path, ValueError, vol(np.float32), target_bits=4, method='planes')
    refused(tmp_path, ValueError, vol(np.uint8), target_ratio=4, method='planes')
    refused(tmp_path, ValueError, vol(np.uint8), target_ratio=4, method='huffman')


@pytest.mark.parametrize('dtype', [np.int32, np.uint32, np.float64, np.int64])
def test_dtypes_without_a_mode(tmp_path, dtype):
    refused(tmp_path, TypeError, vol(dtype), target_bits=4)
    refused(tmp_path, TypeError, vol(dtype), target_ratio=4, target_mode='abs')


def test_modes_fit_their_dtypes(tmp_path):
    for dtype in (np.uint8, np.uint16, np.int8, np.int16):
        assert rate.check_target(np.dtype(dtype), 4, None, None) == 'near'
        assert rate.check_target(np.dtype(dtype), None, 3, 'near') == 'near'
        for mode in ('abs', 'rel'):
            refused(tmp_path, ValueError, vol(dtype), target_bits=4, target_mode=mode)
    assert rate.check_target(np.dtype(np.float32), 4, None, None) == 'abs'
    assert rate.check_target(np.dtype(np.float32), 4, None, 'rel') == 'rel'
    assert rate.check_target(np.dtype(np.float32), None, None, None) is None
    refused(tmp_path, ValueError, vol(np.float32), target_bits=4, target_mode='near')
    for mode in ('psnr', '', 3, True):
        refused(tmp_path, ValueError, vol(np.float32), target_bits=4, target_mode=mode)
        refused(tmp_path, ValueError, vol(np.uint8), target_bits=4, target_mode=mode)


def test_compressed_size_argument_errors():
    P = kom.MeanPredictor(0, 3)
    for method in ('planes', 'huffman'):
        with pytest.raises(ValueError):
            container.compressed_size(vol(np.float32), P, levels=1, method=method)
    for bad in (True, '1e-3', math.nan, 0, -1.0, 2.0 ** -128):
        with pytest.raises(ValueError):
            container.compressed_size(vol(np.float32), P, levels=1, abs_error=bad)
    for bad in (True, '1e-3', math.nan, 0, 1.0, 2.0 ** -25):
        with pytest.raises(ValueError):
            container.compressed_size(vol(np.float32), P, levels=1, rel_error=bad)
    for bad in (True, 1.5, -1, 128):
        with pytest.raises(ValueError):
            container.compressed_size(vol(np.uint8), P, levels=1, max_error=bad)
    for kw in ({'abs_error': 1e-3, 'rel_error': 1e-3}, {'abs_error': 1e-3, 'max_error': 1},
               {'rel_error': 1e-3, 'max_error': 1}):
        with pytest.raises(ValueError):
            container.compressed_size(vol(np.float32), P, levels=1, **kw)
    for kw in ({'abs_error': 1e-3}, {'rel_error': 1e-3}):
        with pytest.raises(TypeError):
            container.compressed_size(vol(np.uint16), P, levels=1, **kw)
    with pytest.raises(TypeError):
        container.compressed_size(vol(np.float32), P, levels=1, max_error=1)
    with pytest.raises(TypeError):
        container.compressed_size(vol(np.int32), P, levels=1, max_error=1)


@pytest.mark.parametrize('M,first,last', [
    (0.0, 0, 0), (math.nan, 0, 0), (math.inf, 0, 0),   # nothing finite to go by: the single rung 0
    (FLT_MAX, 98, 127),                                # ex = 128: ex + 1 clamps to 127
    (SUBNORMAL, -126, -126),                           # ex = -148: both ends clamp to -126, one rung
    (2.0 ** -120, -126, -118),                         # ex = -119: the fine end clamps
    (1.0, -29, 2), (0.75, -30, 1), (12.5, -26, 5), (2.0 ** 126, 97, 127), (2.0 ** 125, 96, 127), (2.0 ** 124, 95, 126)])
def test_abs_ladder_end_points(M, first, last):
    lad = rate.ladder_abs(M)
    assert lad == R.ladder_abs(M) == list(range(first, last + 1))
    assert all(R.E_MIN <= e <= R.E_MAX for e in lad)
    if math.isfinite(M) and M > 0 and last < 127:
        assert M * 2.0 ** -last < 0.5          # the coarse end: every finite value quantises to 0
    if math.isfinite(M) and M > 0 and first > -126:
        assert 2.0 ** first < 2.0 ** (math.frexp(M)[1] - 24)  # the fine end: the step is below the largest values' ulp


def test_rel_and_near_ladders():
    assert rate.ladder_rel() == R.ladder_rel() == list(range(22, -1, -1))
    for dtype, top in ((np.uint8, 127), (np.int8, 127), (np.uint16, 32767), (np.int16, 32767)):
        lad = rate.ladder_near(dtype)
        assert (lad[0], lad[-1], len(lad)) == (0, top, top + 1) == (R.ladder_near(dtype)[0], R.ladder_near(dtype)[-1],
                                                                    len(R.ladder_near(dtype)))
        assert top == kom.near.max_error_limit(dtype)


def test_a_rung_is_coded_by_its_explicit_bound():
    for e in (-126, -9, 0, 127):
        assert rate.bound_of('abs', e) == ('abs_error', R.bound_kw('abs', e)['abs_error'])
        assert kom.quant.exponent(rate.bound_of('abs', e)[1]) == e
    for m in range(23):
        assert rate.bound_of('rel', m) == ('rel_error', R.bound_kw('rel', m)['rel_error'])
        assert kom.quant.mantissa_bits(rate.bound_of('rel', m)[1]) == m
    assert rate.bound_of('near', 5) == ('max_error', 5)
