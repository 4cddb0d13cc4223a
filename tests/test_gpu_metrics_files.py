"""Quality figures of compressed files against tests/metrics_spec.py: the ``'mse'`` / ``'psnr'`` /
``'value_range'`` of every lossy ``compress`` result are the spec's on what ``decompress`` returns,
``container.compare`` agrees, exceptions are never mismatches, and ``compress(target_psnr=...)`` writes the
explicit-bound file of the rung the rule names -- on ``quant_spec.spec_field()`` (1 x 40 x 48 x 56 x 1,
MeanPredictor(0)) and on a uint16 field of that shape."""

import filecmp
import math
import os

import numpy as np
import pytest
import torch

import metrics_spec as M
import near_spec as NS
import quant_spec as Q
import signed_spec as SS

pytestmark = pytest.mark.gpu

SHAPE = (1, 40, 48, 56, 1)
LEVELS = 2
_DATA = {}


def data(name):
    if not _DATA:
        _DATA['f32'] = Q.spec_field()
        _DATA['u16'] = NS.noisy_field(SHAPE, np.uint16, seed=1)
        _DATA['i8'] = NS.noisy_field((1, 20, 24, 33, 1), np.int8, seed=2)
        assert _DATA['f32'].shape == SHAPE
    return _DATA[name]


def exceptions_field(shape=(1, 20, 24, 33, 1), seed=0):
    """A smooth float32 field under a little noise with a NaN block, both infinities, NaN payloads and one
    value past the int32 range of every step used here (test_gpu_quant_files.field)."""
    rng = np.random.default_rng(seed)
    x = (3.0 * SS.smooth_field(shape[1:-1], seed) + 0.01 * rng.standard_normal(shape[1:-1])).astype(np.float32)
    x = x.reshape(shape).copy()
    x[(0, *[slice(s // 3, s // 3 + 3) for s in shape[1:4]])] = np.nan
    f = x.reshape(-1)
    f[[0, 7, f.size - 1]] = [np.inf, -np.inf, 3e38]
    f.view(np.uint32)[[f.size // 2, f.size // 2 + 1]] = [0x7fc00001, 0xffc12345]
    return x


def agrees(got, want, n, is_float):
    """``mse`` / ``psnr`` / ``value_range`` of a result (or a ``compare``) against the spec's."""
    assert got['value_range'] == want['value_range']
    if is_float:
        assert abs(got['mse'] - want['mse']) <= n * 2.0 ** -52 * want['mse']
    else:
        assert got['mse'] == want['mse']
    assert abs(got['psnr'] - want['psnr']) <= 1e-9 or got['psnr'] == want['psnr']


LOSSY = [('abs', 'f32', {'abs_error': 2.0 ** -8}), ('abs-coarse', 'f32', {'abs_error': 0.3}),
         ('rel', 'f32', {'rel_error': 2.0 ** -10}), ('near-u16', 'u16', {'max_error': 5}), ('near-i8', 'i8', {'max_error': 3})]


@pytest.mark.parametrize('case', LOSSY, ids=[c[0] for c in LOSSY])
def test_lossy_results_agree_with_the_spec(kom, tmp_path, case):
    _, name, bound = case
    x = data(name)
    path = str(tmp_path / 'f.kmp')
    out = kom.container.compress(path, x, kom.MeanPredictor(0, 3), levels=LEVELS, **bound)
    r = kom.container.decompress(path)
    want = M.compare(x, r)
    print(f'{case[0]}: psnr {out["psnr"]!r} (spec {want["psnr"]!r}), mse {out["mse"]!r} (spec {want["mse"]!r})')
    is_float = x.dtype == np.float32
    agrees(out, want, x.size, is_float)
    assert math.isfinite(out['psnr']) and out['mse'] > 0
    assert want['peak'] == (want['value_range'] if is_float else 2 ** (8 * x.dtype.itemsize) - 1)
    full = kom.container.compare(path, x)
    agrees(full, want, x.size, is_float)
    assert (full['psnr'], full['mse'], full['value_range']) == (out['psnr'], out['mse'], out['value_range'])
    assert full['count'] == x.size and full['mismatch'] == 0 and full['max_abs_error'] == want['max_abs_error']
    if 'max_abs_error' in out:  # the record's max_abs is the bound check's own figure
        assert full['max_abs_error'] == out['max_abs_error']
    assert kom.container.compare(path, torch.from_numpy(x.copy()).cuda(), peak=7.5) == \
        kom.metrics.compare(x, r, peak=7.5)
    with pytest.raises(ValueError):
        kom.container.compare(path, x[:, :-1])
    with pytest.raises(TypeError):
        kom.container.compare(path, x.view(np.uint32 if is_float else {1: np.uint8, 2: np.int16}[x.dtype.itemsize]))
    with pytest.raises(ValueError):
        kom.container.compare(path, x, peak=0)


def test_lossless_results_hold_the_figures_without_a_launch(kom, tmp_path):
    for name in ('f32', 'u16'):
        out = kom.container.compress(str(tmp_path / f'{name}.kmp'), data(name), kom.MeanPredictor(0, 3), levels=LEVELS)
        assert out['mse'] == 0.0 and out['psnr'] == math.inf
        assert kom.container.compare(str(tmp_path / f'{name}.kmp'), data(name))['psnr'] == math.inf


@pytest.mark.parametrize('bound', [{'abs_error': 1e-3}, {'rel_error': 1e-3}], ids=['abs', 'rel'])
def test_exceptions_are_not_mismatches(kom, tmp_path, bound):
    x = exceptions_field()
    path = str(tmp_path / 'e.kmp')
    out = kom.container.compress(path, x, kom.MeanPredictor(0, 3), levels=LEVELS, **bound)
    assert out['exceptions'] > 0
    r = kom.container.decompress(path)
    want = M.compare(x, r)
    full = kom.container.compare(path, x)
    assert full['mismatch'] == want['mismatch'] == 0
    assert full['count'] == want['count'] == int(np.isfinite(x).sum()) < x.size  # the finite value past the range is compared
    agrees(out, want, x.size, True)
    agrees(full, want, x.size, True)
    if 'max_abs_error' in out:
        assert full['max_abs_error'] == out['max_abs_error']


@pytest.fixture(scope='module')
def spec_psnr():
    """The spec's PSNR of a rung of the 'abs' ladder on the spec field, computed when first asked."""
    known = {}

    def at(e):
        if e not in known:
            n, exc = Q.quantise(data('f32'), e)
            known[e] = M.compare(data('f32'), Q.restore(n, e, exc))['psnr']
        return known[e]
    return at


@pytest.mark.parametrize('target,e', [(60, -7), (90, -12)])
def test_targets_on_the_spec_field(kom, tmp_path, spec_psnr, target, e):
    x, P = data('f32'), kom.MeanPredictor(0, 3)
    explicit = kom.container.compress(str(tmp_path / 'explicit.kmp'), x, P, levels=LEVELS, abs_error=2.0 ** (e - 1))
    out = kom.container.compress(str(tmp_path / 't.kmp'), x, P, levels=LEVELS, target_psnr=target)
    print(f'target {target} dB: abs_error {out["abs_error"]}, psnr {out["psnr"]!r}, probes {out["probes"]}')
    assert filecmp.cmp(str(tmp_path / 't.kmp'), str(tmp_path / 'explicit.kmp'), shallow=False)
    assert {k: out[k] for k in explicit} == explicit and set(out) - set(explicit) == {'target_psnr', 'probes'}
    assert out['target_psnr'] == target and out['abs_error'] == 2.0 ** (e - 1)
    ladder = list(range(-29, 3))
    assert 1 <= len(out['probes']) <= 2 + math.ceil(math.log2(len(ladder)))
    want, probes = M.search_quality(lambda k: spec_psnr(ladder[k]), len(ladder), target)
    assert ladder[want] == e and [p[0] for p in out['probes']] == [ladder[k] for k, _ in probes]
    for rung, psnr in out['probes']:
        assert abs(psnr - spec_psnr(rung)) <= 1e-9
    assert out['psnr'] >= target > spec_psnr(e + 1) and abs(out['psnr'] - spec_psnr(e)) <= 1e-9
    assert not [f for f in os.listdir(tmp_path) if '.tmp' in f]
    # the default mode, named, and a device input: the same file
    again = kom.container.compress(str(tmp_path / 'again.kmp'), torch.from_numpy(x).cuda(), P, levels=LEVELS,
                                   target_psnr=float(target), target_mode='abs')
    assert filecmp.cmp(str(tmp_path / 'again.kmp'), str(tmp_path / 'explicit.kmp'), shallow=False)
    assert again['probes'] == out['probes']


GUARANTEE = [('rel', 'f32', 75.0, 'rel_error'), ('near-u16', 'u16', 70.0, 'max_error'), ('near-i8', 'i8', 38.0, 'max_error')]


@pytest.mark.parametrize('case', GUARANTEE, ids=[c[0] for c in GUARANTEE])
def test_rel_and_near_targets_keep_the_guarantee(kom, tmp_path, case):
    """The rung written meets the target and its coarser neighbour misses it, both judged by the spec on
    what ``decompress`` returns."""
    _, name, target, key = case
    x, P = data(name), kom.MeanPredictor(0, 3)
    mode = 'rel' if key == 'rel_error' else 'near'
    path = str(tmp_path / 't.kmp')
    out = kom.container.compress(path, x, P, levels=LEVELS, target_psnr=target, target_mode=mode)
    L = 23 if mode == 'rel' else (1 << (8 * x.dtype.itemsize - 1))
    print(f'{case[0]} target {target} dB: {key} {out[key]}, psnr {out["psnr"]!r}, {len(out["probes"])} probes')
    assert len(out['probes']) <= 2 + math.ceil(math.log2(L)) and out['target_psnr'] == target
    here = M.compare(x, kom.container.decompress(path))['psnr']
    assert here >= target and abs(here - out['psnr']) <= 1e-9
    coarser = {'rel_error': out[key] * 2} if mode == 'rel' else {'max_error': out[key] + 1}
    explicit = str(tmp_path / 'explicit.kmp')
    same = kom.container.compress(explicit, x, P, levels=LEVELS, **{key: out[key]})
    assert filecmp.cmp(path, explicit, shallow=False) and {k: out[k] for k in same} == same
    kom.container.compress(str(tmp_path / 'coarser.kmp'), x, P, levels=LEVELS, **coarser)
    there = M.compare(x, kom.container.decompress(str(tmp_path / 'coarser.kmp')))['psnr']
    print(f'  the spec: {here!r} dB at the rung, {there!r} dB at its coarser neighbour')
    assert there < target


def test_an_unreachable_target_writes_nothing(kom, tmp_path):
    path = str(tmp_path / 'never.kmp')
    for mode in ('abs', 'rel'):
        with pytest.raises(ValueError) as e:
            kom.container.compress(path, data('f32'), kom.MeanPredictor(0, 3), levels=LEVELS, target_psnr=1000,
                                   target_mode=mode)
        assert 'dB' in str(e.value) and 'finest' in str(e.value)
        assert not os.path.exists(path) and os.listdir(tmp_path) == []
    # integer samples: rung 0 is lossless, so every target is met
    out = kom.container.compress(path, data('i8'), kom.MeanPredictor(0, 3), levels=LEVELS, target_psnr=1000)
    assert out['max_error'] == 0 and out['psnr'] == math.inf and (0, math.inf) in out['probes']
    assert np.array_equal(kom.container.decompress(path), data('i8'))
