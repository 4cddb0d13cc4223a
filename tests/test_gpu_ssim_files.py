"""SSIM of compressed files against tests/ssim_spec.py: ``container.ssim`` is the spec's on what ``decompress``
returns, and ``compress(target_ssim=...)`` writes the explicit-bound file of a rung that meets the target while
its coarser neighbour does not -- on a 1 x 24 x 28 x 32 x 1 corner of ``quant_spec.spec_field()``, a uint16 field
of that shape, a NaN slab and three frames of ``delta_spec.sequence``."""

import filecmp
import math
import os

import numpy as np
import pytest
import torch

import delta_spec as D
import near_spec as NS
import quant_spec as Q
import ssim_spec as S

pytestmark = pytest.mark.gpu

SHAPE = (1, 24, 28, 32, 1)
LEVELS = 2
_DATA = {}


def data(name):
    if not _DATA:
        _DATA['f32'] = np.ascontiguousarray(Q.spec_field()[:, :24, :28, :32])
        _DATA['u16'] = NS.noisy_field(SHAPE, np.uint16, seed=1)
        slab = _DATA['f32'].copy()
        slab[0, 9:14] = np.nan
        _DATA['slab'] = slab
        _DATA['frames'] = D.sequence(1.0, 0.02, frames=3, shape=SHAPE[1:4])
        assert _DATA['f32'].shape == SHAPE and _DATA['frames'].shape == (3,) + SHAPE[1:]
    return _DATA[name]


def spec_of(x, r):
    return S.ssim(S.items(x), S.items(r))


def close(got, want, is_float):
    tol = S.TOL_F32 if is_float else S.TOL_INT
    assert (got['windows'], got['skipped'], got['peak'], got['base']) == (want['windows'], want['skipped'], want['peak'], want['base'])
    assert abs(got['ssim'] - want['ssim']) <= tol and abs(got['min_ssim'] - want['min_ssim']) <= tol


CASES = [('abs', 'f32', {'abs_error': 2.0 ** -5}), ('rel', 'f32', {'rel_error': 2.0 ** -8}), ('near', 'u16', {'max_error': 40})]


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_container_ssim_is_the_spec_on_what_decompress_returns(kom, tmp_path, case):
    _, name, bound = case
    x, path = data(name), str(tmp_path / 'f.kmp')
    kom.container.compress(path, x, kom.MeanPredictor(0, 3), levels=LEVELS, **bound)
    r = kom.container.decompress(path)
    want = spec_of(x, r)
    got = kom.container.ssim(path, x)
    print(f'{case[0]}: ssim {got["ssim"]!r} (spec {want["ssim"]!r}), min {got["min_ssim"]!r}, windows {got["windows"]}')
    close(got, want, x.dtype == np.float32)
    assert want['windows'] == 18 * 22 * 26 and 0 < got['ssim'] < 1
    assert kom.container.ssim(path, torch.from_numpy(x.copy()).cuda(), peak=7.5) == kom.metrics.ssim(x, r, peak=7.5)
    with pytest.raises(ValueError):
        kom.container.ssim(path, x[:, :-1])
    with pytest.raises(TypeError):
        kom.container.ssim(path, x.view(np.uint32 if x.dtype == np.float32 else np.int16))
    with pytest.raises(ValueError):
        kom.container.ssim(path, x, peak=0)


# uint16 samples are judged against the peak 65535: on a field that spans 1649 .. 2306 even the coarsest rung keeps
# 0.998, so the 'near' target sits above it
TARGETS = [('abs', 'f32', 0.99, 'abs_error', {}), ('rel', 'f32', 0.99, 'rel_error', {}), ('near', 'u16', 0.9999, 'max_error', {}),
           ('abs-runs', 'slab', 0.995, 'abs_error', {'exceptions': 'runs'}),
           ('abs-delta', 'frames', 0.98, 'abs_error', {'temporal': 'delta'})]


@pytest.mark.parametrize('case', TARGETS, ids=[c[0] for c in TARGETS])
def test_target_ssim_keeps_the_guarantee(kom, tmp_path, case):
    """The file is the explicit-bound file of the chosen rung, byte for byte; judged by ``container.ssim`` (and
    the spec) on what ``decompress`` returns it meets the target and its coarser neighbour does not."""
    tag, name, target, key, extra = case
    x, P = data(name), kom.MeanPredictor(0, 3)
    mode = {'abs_error': 'abs', 'rel_error': 'rel', 'max_error': 'near'}[key]
    path, explicit = str(tmp_path / 't.kmp'), str(tmp_path / 'explicit.kmp')
    out = kom.container.compress(path, x, P, levels=LEVELS, target_ssim=target, target_mode=mode, **extra)
    L = {'abs': 32, 'rel': 23, 'near': 1 << 15}[mode]
    print(f'{tag} target {target}: {key} {out[key]}, ssim {out["ssim"]!r}, {len(out["probes"])} probes {out["probes"]}')
    assert 1 <= len(out['probes']) <= 2 + math.ceil(math.log2(L)) and out['target_ssim'] == target
    same = kom.container.compress(explicit, x, P, levels=LEVELS, **{key: out[key]}, **extra)
    assert filecmp.cmp(path, explicit, shallow=False)
    assert {k: out[k] for k in same} == same and set(out) - set(same) == {'ssim', 'target_ssim', 'probes'}
    here = kom.container.ssim(path, x)
    close(here, spec_of(x, kom.container.decompress(path)), x.dtype == np.float32)
    assert here['ssim'] >= target and here['ssim'] == out['ssim']
    if tag == 'abs-runs':
        assert out['exceptions'] > 0 and here['skipped'] > 0
    if tag == 'abs-delta':
        assert out['temporal'] == 'delta' and here['windows'] == 3 * 18 * 22 * 26
    coarser = {key: out[key] + 1} if mode == 'near' else {key: out[key] * 2}
    kom.container.compress(str(tmp_path / 'coarser.kmp'), x, P, levels=LEVELS, **coarser, **extra)
    there = kom.container.ssim(str(tmp_path / 'coarser.kmp'), x)['ssim']
    print(f'  at the rung {here["ssim"]!r}, at its coarser neighbour {there!r}')
    assert there < target
    assert not [f for f in os.listdir(tmp_path) if '.tmp' in f]


def test_the_default_mode_and_a_device_input(kom, tmp_path):
    x, P = data('f32'), kom.MeanPredictor(0, 3)
    a = kom.container.compress(str(tmp_path / 'a.kmp'), x, P, levels=LEVELS, target_ssim=0.99)
    b = kom.container.compress(str(tmp_path / 'b.kmp'), torch.from_numpy(x).cuda(), P, levels=LEVELS, target_ssim=0.99,
                               target_mode='abs', method='rice')
    assert filecmp.cmp(str(tmp_path / 'a.kmp'), str(tmp_path / 'b.kmp'), shallow=False) and a['probes'] == b['probes']
    # the rule's own rung: the coarsest-leaning one whose spec SSIM meets the target
    e = int(math.log2(a['abs_error'])) + 1  # the result holds the effective bound 2^(e - 1)
    n, exc = Q.quantise(x, e)
    assert S.ssim(S.items(x), S.items(Q.restore(n, e, exc)))['ssim'] >= 0.99
    n, exc = Q.quantise(x, e + 1)
    assert S.ssim(S.items(x), S.items(Q.restore(n, e + 1, exc)))['ssim'] < 0.99


def test_a_target_of_one_on_integers_gives_the_lossless_file(kom, tmp_path):
    x, P = data('u16'), kom.MeanPredictor(0, 3)
    out = kom.container.compress(str(tmp_path / 't.kmp'), x, P, levels=LEVELS, target_ssim=1.0)
    kom.container.compress(str(tmp_path / 'lossless.kmp'), x, P, levels=LEVELS)
    assert filecmp.cmp(str(tmp_path / 't.kmp'), str(tmp_path / 'lossless.kmp'), shallow=False)
    assert out['max_error'] == 0 and out['ssim'] == 1.0 and (0, 1.0) in out['probes']
    assert np.array_equal(kom.container.decompress(str(tmp_path / 't.kmp')), x)


def test_an_unreachable_target_writes_nothing(kom, tmp_path):
    path = str(tmp_path / 'never.kmp')
    # the finest 'rel' rung keeps 22 of the 23 mantissa bits: around 1000 that is an error of 6e-5 on a range of
    # 2.3, an SSIM about 1e-7 below 1 -- far outside any rounding, so 1.0 is out of reach
    x = (data('f32') + np.float32(1000)).astype(np.float32)
    with pytest.raises(ValueError) as e:
        kom.container.compress(path, x, kom.MeanPredictor(0, 3), levels=LEVELS, target_ssim=1.0, target_mode='rel')
    assert 'SSIM' in str(e.value) and 'finest' in str(e.value)
    assert not os.path.exists(path) and os.listdir(tmp_path) == []
