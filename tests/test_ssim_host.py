"""SSIM, the host side: the header's constants are ``_lib``'s, ``metrics.ssim_summary`` is tests/ssim_spec.py's
arithmetic, and every argument error of ``metrics.ssim``, ``container.ssim``, ``compress(target_ssim=...)`` and
``rate.check_target`` is raised before the device is touched (these tests run without a GPU)."""

import math
import os
import re

import numpy as np
import pytest

import kompressor_amd as kom
from kompressor_amd import _lib, container, metrics, rate

HERE = os.path.dirname(os.path.abspath(__file__))
BAD_NUMBERS = [True, False, '4', math.nan, math.inf, -math.inf, 0, 0.0, -1, -0.5, 10 ** 400, [4], b'4']


def vol(dtype, side=8):
    return np.zeros((1, side, side, side, 1), dtype)


def refused(tmp_path, exc, x, **kw):
    with pytest.raises(exc):
        container.compress(str(tmp_path / 'x.kmp'), x, kom.MeanPredictor(0, x.ndim - 2), levels=1, **kw)
    assert not os.listdir(tmp_path)


def test_the_headers_constants_are_the_bindings():
    with open(os.path.join(HERE, '..', 'include', 'kompressor_hip.h')) as f:
        text = f.read()
    define = {k: v.strip() for k, v in re.findall(r'#define (KMP_SSIM_[A-Z_]+) (.+)', text)}
    assert int(re.search(r'KMP_CODER_SSIM = (\d+)', text).group(1)) == _lib.CODER_SSIM == 14
    assert int(define['KMP_SSIM_GROUPS']) == _lib.SSIM_GROUPS
    assert define['KMP_SSIM_BYTES'] == '(64 * (2 + KMP_SSIM_GROUPS))' and _lib.SSIM_BYTES == 64 * (2 + _lib.SSIM_GROUPS)
    assert (int(define['KMP_SSIM_TILE_D']), int(define['KMP_SSIM_TILE_H']), int(define['KMP_SSIM_TILE_W'])) == \
        (_lib.SSIM_TILE_D, _lib.SSIM_TILE_H, _lib.SSIM_TILE_W)
    assert _lib.ssim_groups(1) == 1 and _lib.ssim_groups(257) == 2 and _lib.ssim_groups(1 << 40) == _lib.SSIM_GROUPS
    assert 'kmp_code' in _lib.EXPORTED and not any('ssim' in name for name in _lib.EXPORTED)  # no new entry point
    assert callable(metrics.ssim) and callable(metrics.d_ssim) and callable(container.ssim)
    assert 'target_ssim' in container.compress.__code__.co_varnames


def test_summary_is_the_host_arithmetic():
    f = lambda v: int(np.array([v], np.float64).view(np.uint64)[0])  # noqa: E731
    words = np.array([4, 3, f(3.5), f(0.25), 0, 0, 0, 0], np.uint64)
    assert metrics.ssim_summary(words) == {'ssim': 0.875, 'min_ssim': 0.25, 'windows': 4, 'skipped': 3}
    none = metrics.ssim_summary(np.array([0, 9, f(0.0), f(math.inf), 0, 0, 0, 0], np.uint64))
    assert math.isnan(none['ssim']) and none['min_ssim'] == math.inf and none['windows'] == 0 and none['skipped'] == 9
    with pytest.raises(ValueError):
        metrics.ssim_summary(np.array([0, 0, f(0.0), f(math.inf), 1, 0, 0, 0], np.uint64))
    assert metrics.ssim_dims((2, 9, 8, 3)) == (6, 1, 9, 8) and metrics.ssim_dims((2, 7, 9, 8, 1)) == (2, 7, 9, 8)
    c1, c2 = metrics.ssim_constants(255.0)
    assert (c1, c2) == ((0.01 * 255.0) ** 2, (0.03 * 255.0) ** 2)


@pytest.mark.parametrize('dtype', [np.int32, np.uint32, np.float64, np.int64, np.float16, bool])
def test_ssim_refuses_other_dtypes(dtype):
    with pytest.raises(TypeError):
        metrics.ssim(np.zeros((1, 8, 8, 1), dtype), np.zeros((1, 8, 8, 1), dtype))


def test_ssim_argument_errors():
    x = np.zeros((1, 8, 9, 1), np.float32)
    for other in (np.uint8, np.int16, np.float64):
        with pytest.raises(TypeError):
            metrics.ssim(x, np.zeros(x.shape, other))
        with pytest.raises(TypeError):
            metrics.ssim(np.zeros(x.shape, other), x)
    for shape in ((1, 9, 8, 1), (1, 8, 9), (1, 8, 9, 2), (72,)):
        with pytest.raises(ValueError):
            metrics.ssim(x, np.zeros(shape, np.float32))
    for shape in ((8, 9), (1, 8, 9), (72,), (1, 1, 8, 8, 9, 1), ()):  # a rank other than 4 / 5
        with pytest.raises(ValueError):
            metrics.ssim(np.zeros(shape, np.uint8), np.zeros(shape, np.uint8))
    for shape in ((1, 6, 9, 1), (1, 9, 6, 1), (2, 6, 9, 9, 1), (2, 9, 6, 9, 1), (2, 9, 9, 6, 1), (1, 1, 9, 9, 1), (1, 0, 9, 1)):
        with pytest.raises(ValueError):
            metrics.ssim(np.zeros(shape, np.uint16), np.zeros(shape, np.uint16))  # an extent below the window
    for bad in BAD_NUMBERS:
        with pytest.raises(ValueError):
            metrics.ssim(x, x, peak=bad)


class _File:
    """What ``container.info`` says of a file, without one."""

    def __init__(self, monkeypatch, dtype, shape):
        monkeypatch.setattr(container, 'info', lambda path: {'sample_dtype': dtype, 'shape': list(shape)})


def test_container_ssim_argument_errors(monkeypatch):
    _File(monkeypatch, 'uint16', (1, 8, 9, 10, 1))
    x = np.zeros((1, 8, 9, 10, 1), np.uint16)
    with pytest.raises(TypeError):
        container.ssim('f.kmp', x.view(np.int16))
    with pytest.raises(ValueError):
        container.ssim('f.kmp', x[:, :-1])
    for bad in BAD_NUMBERS:
        with pytest.raises(ValueError):
            container.ssim('f.kmp', x, peak=bad)
    _File(monkeypatch, 'int32', (1, 8, 9, 10, 1))
    with pytest.raises(TypeError):
        container.ssim('f.kmp', x.astype(np.int32))  # no SSIM for int32 samples
    _File(monkeypatch, 'uint16', (1, 8, 6, 10, 1))
    with pytest.raises(ValueError):
        container.ssim('f.kmp', np.zeros((1, 8, 6, 10, 1), np.uint16))  # an extent below the window


@pytest.mark.parametrize('bad', BAD_NUMBERS + [1.0000001, 2, 1e9])
def test_bad_target_ssim(bad, tmp_path):
    for x in (vol(np.float32), vol(np.uint16)):
        refused(tmp_path, ValueError, x, target_ssim=bad)


@pytest.mark.parametrize('other', [{'target_bits': 4}, {'target_ratio': 8}, {'target_psnr': 60}, {'abs_error': 1e-3},
                                   {'rel_error': 1e-3}, {'max_error': 1}])
def test_target_ssim_stands_alone(tmp_path, other):
    for x in (vol(np.float32), vol(np.uint16)):
        refused(tmp_path, ValueError, x, target_ssim=0.99, **other)


def test_target_ssim_needs_room_for_a_window(tmp_path):
    for shape in ((1, 6, 8, 8, 1), (1, 8, 6, 8, 1), (1, 8, 8, 6, 1), (1, 5, 5, 5, 1)):
        refused(tmp_path, ValueError, np.zeros(shape, np.float32), target_ssim=0.99)
        refused(tmp_path, ValueError, np.zeros(shape, np.uint8), target_ssim=0.99)
    refused(tmp_path, ValueError, np.zeros((2, 6, 9, 1), np.uint8), target_ssim=0.99)


def test_target_ssim_modes_fit_their_dtypes(tmp_path):
    for dtype in (np.uint8, np.uint16, np.int8, np.int16):
        assert rate.check_target(np.dtype(dtype), None, None, None, target_ssim=0.9) == 'near'
        assert rate.check_target(np.dtype(dtype), None, None, 'near', 'planes', target_ssim=1) == 'near'  # any method
        for mode in ('abs', 'rel'):
            refused(tmp_path, ValueError, vol(dtype), target_ssim=0.9, target_mode=mode)
    assert rate.check_target(np.dtype(np.float32), None, None, None, target_ssim=0.9) == 'abs'
    assert rate.check_target(np.dtype(np.float32), None, None, 'rel', 'planes', target_ssim=1.0) == 'rel'
    refused(tmp_path, ValueError, vol(np.float32), target_ssim=0.9, target_mode='near')
    for mode in ('ssim', '', 3, True):
        refused(tmp_path, ValueError, vol(np.float32), target_ssim=0.9, target_mode=mode)
    for dtype in (np.int32, np.uint32, np.float64, np.int64):
        refused(tmp_path, TypeError, vol(dtype), target_ssim=0.9)
    refused(tmp_path, ValueError, vol(np.uint16), target_ssim=0.9, temporal='delta')  # as for every near target
    refused(tmp_path, ValueError, vol(np.uint16), target_ssim=0.9, exceptions='runs')
    refused(tmp_path, ValueError, vol(np.float32), target_ssim=0.9, key_interval=2)


def test_check_target_keeps_its_callers_and_its_messages():
    """``target_ssim`` is a last keyword with a default: today's calls mean, and say, what they did."""
    f32 = np.dtype(np.float32)
    assert rate.check_target.__code__.co_varnames[:rate.check_target.__code__.co_argcount][-2:] == ('target_psnr', 'target_ssim')
    assert rate.check_target(f32, None, None, None) is None
    assert rate.check_target(f32, 4, None, None, 'rice', 0, None, None) == 'abs'
    assert rate.check_target(f32, None, None, None, 'planes', 0, None, None, 60) == 'abs'
    with pytest.raises(ValueError, match='^target_mode needs target_bits, target_ratio or target_psnr$'):
        rate.check_target(f32, None, None, 'abs')
    with pytest.raises(ValueError, match='^give one of target_bits, target_ratio and target_psnr, not target_bits and target_psnr$'):
        rate.check_target(f32, 4, None, None, target_psnr=60)
    with pytest.raises(ValueError, match='^target_psnr chooses the bound: not with max_error, abs_error or rel_error$'):
        rate.check_target(f32, None, None, None, abs_error=1e-3, target_psnr=60)
    with pytest.raises(ValueError, match="need method='rice'"):
        rate.check_target(f32, 4, None, None, 'planes')
    with pytest.raises(ValueError, match='target_ssim'):
        rate.check_target(f32, 4, None, None, target_ssim=0.5)
    with pytest.raises(ValueError, match=r'\(0, 1\]'):
        rate.check_target(f32, None, None, None, target_ssim=1.5)
