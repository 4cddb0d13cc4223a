"""Masked float32 fields, the host side: every argument error is raised before the device is
touched (these tests run without a GPU), a version-7 header is accepted or refused by its metadata alone,
and ``plan_region`` reads the four run arrays whole."""

import json
import os

import numpy as np
import pytest
import torch

import kompressor_amd as kom
from kompressor_amd import _lib, container, quant


def test_exported():
    assert (_lib.CODER_FILL, _lib.CODER_RUNS) == (11, 12)
    assert _lib.FILL_BYTES == 16 * _lib.FILL_GROUPS and _lib.FILL_BYTES % 8 == 0
    assert container.VERSION_RUNS == 7
    # the span of a workgroup is a function of the count alone: whole tiles, at most FILL_GROUPS spans
    for n in (1, 2048, 2049, 4097, 2048 * 1024, 2048 * 1024 + 1, 10 ** 9):
        span = _lib.fill_span(n)
        assert span % _lib.FILL_TILE == 0 and span >= _lib.FILL_TILE and -(-n // span) <= _lib.FILL_GROUPS
    assert _lib.fill_span(4096) == 2048 and _lib.fill_span(2048 * 1024 + 1) == 4096


X = np.zeros((1, 5, 5, 5, 1), np.float32)


@pytest.mark.parametrize('bad', ['Runs', 'run', '', 'LIST', None, 0, 1, True, b'runs', ['runs'], ('list',)])
def test_bad_exceptions_keyword(bad, tmp_path):
    pred = kom.MeanPredictor(0, 3)
    for kw in ({'abs_error': 1e-3}, {'rel_error': 1e-3}, {'target_bits': 4.0}, {'target_psnr': 40.0}, {}):
        with pytest.raises(ValueError):
            container.compress(str(tmp_path / 'x.kmp'), X, pred, levels=1, exceptions=bad, **kw)
    for kw in ({'abs_error': 1e-3}, {'rel_error': 1e-3}, {}):
        with pytest.raises(ValueError):
            container.compressed_size(X, pred, levels=1, exceptions=bad, **kw)
    assert not os.listdir(tmp_path)


def test_runs_need_a_float32_bound(tmp_path):
    pred = kom.MeanPredictor(0, 3)
    u16 = np.zeros((1, 5, 5, 5, 1), np.uint16)
    for x, kw in ((X, {}), (u16, {}), (u16, {'max_error': 2}), (u16, {'target_bits': 4.0}),
                  (u16, {'target_psnr': 40.0}), (u16, {'target_ratio': 2.0, 'target_mode': 'near'})):
        with pytest.raises(ValueError):
            container.compress(str(tmp_path / 'x.kmp'), x, pred, levels=1, exceptions='runs', **kw)
    for x, kw in ((X, {}), (u16, {}), (u16, {'max_error': 2})):
        with pytest.raises(ValueError):
            container.compressed_size(x, pred, levels=1, exceptions='runs', **kw)
    assert not os.listdir(tmp_path)


def test_quant_argument_errors():
    idx, bits = np.array([1, 2], np.int64), np.array([5, 5], np.uint32)
    for bad in ((idx.astype(np.int32), bits), (idx, bits.astype(np.int32)), (idx, bits.view(np.float32))):
        with pytest.raises(TypeError):
            quant.runs(bad)
        with pytest.raises(TypeError):
            quant.fill(np.zeros(4, np.int16), bad)
    for bad in ((idx, bits[:1]), (idx.reshape(1, 2), bits.reshape(1, 2))):
        with pytest.raises(ValueError):
            quant.runs(bad)
    for dtype in (np.float32, np.uint16, np.int64, np.int8):
        with pytest.raises(TypeError):
            quant.fill(np.zeros(4, dtype), (idx, bits))
    u = np.zeros(2, np.uint32)
    with pytest.raises(TypeError):
        quant.exceptions_from_runs(u, u, u.astype(np.int32), u)
    with pytest.raises(TypeError):
        quant.exceptions_from_runs(torch.zeros(2, dtype=torch.int64), u, u, u)
    with pytest.raises(ValueError):
        quant.exceptions_from_runs(u, u, u[:1], u)
    with pytest.raises(ValueError):
        quant.exceptions_from_runs(u.reshape(1, 2), u.reshape(1, 2), u.reshape(1, 2), u.reshape(1, 2))


# ---- headers ------------------------------------------------------------------------------------------

_QUANT = {'exp': -9, 'dtype': 'int16', 'exceptions': 12}
_PREC = {'bits': 6, 'dtype': 'int16', 'exceptions': 12}


def _header(tmp_path, version, **meta_over):
    meta = {'format': 'kompressor_amd', 'ndim': 3, 'padding': 0, 'method': 'rice', 'sample_dtype': 'float32',
            'levels': [{'highres_shape': [1, 5, 5, 5, 1], 'dims': [0, 0, 0]}], 'lowres_shape': [1, 3, 3, 3, 1],
            'predictor': {'kind': 'mean', 'padding': 0, 'ndim': 3}, 'bundle_bytes': 0, 'crc32': 0,
            'quant': _QUANT, 'exception_runs': 3}
    meta.update(meta_over)
    meta = {k: v for k, v in meta.items() if v is not ...}
    js = json.dumps(meta, separators=(',', ':')).encode()
    js += b' ' * (-len(js) % 8)
    path = tmp_path / f'v{version}.kmp'
    path.write_bytes(container._HEAD.pack(container.MAGIC, version, 0, len(js)) + js)
    return str(path)


def test_version7_header(tmp_path):
    info = container.info(_header(tmp_path, 7))
    assert info['version'] == 7 and info['sample_dtype'] == 'float32' and info['shape'] == (1, 5, 5, 5, 1)
    assert info['abs_error'] == 2.0 ** -10 and info['quant_dtype'] == 'int16'
    assert info['exceptions'] == 12 and info['exception_runs'] == 3 and 'rel_error' not in info
    info = container.info(_header(tmp_path, 7, quant=..., prec=_PREC, exception_runs=12))
    assert info['version'] == 7 and info['rel_error'] == 2.0 ** -7 and info['exception_runs'] == 12
    assert 'abs_error' not in info
    assert container.info(_header(tmp_path, 7, exception_runs=1))['exception_runs'] == 1
    assert container.level_shapes(_header(tmp_path, 7)) == [(1, 5, 5, 5, 1), (1, 3, 3, 3, 1)]
    # the files without runs say nothing of them
    assert 'exception_runs' not in container.info(_header(tmp_path, 5, exception_runs=...))
    assert 'exception_runs' not in container.info(_header(tmp_path, 6, quant=..., prec=_PREC, exception_runs=...))


@pytest.mark.parametrize('over', [
    {'exception_runs': ...}, {'exception_runs': None}, {'exception_runs': True}, {'exception_runs': False},
    {'exception_runs': 3.0}, {'exception_runs': '3'}, {'exception_runs': [3]}, {'exception_runs': 0},
    {'exception_runs': -1}, {'exception_runs': 13},
    {'quant': dict(_QUANT, exceptions=0), 'exception_runs': 1}, {'quant': dict(_QUANT, exceptions=0), 'exception_runs': 0},
    {'quant': ...}, {'quant': _QUANT, 'prec': _PREC}, {'quant': None}, {'quant': None, 'prec': None},
    {'quant': ..., 'prec': None}, {'quant': {}}, {'quant': dict(_QUANT, exp=200)}, {'quant': dict(_QUANT, dtype='int8')},
    {'quant': dict(_QUANT, exceptions='12')}, {'quant': ..., 'prec': dict(_PREC, bits=23)},
    {'max_error': 0}, {'max_error': 2}, {'max_error': None}, {'quant': ..., 'prec': _PREC, 'max_error': 1},
    {'sample_dtype': 'int16'}, {'sample_dtype': 'uint32'}, {'sample_dtype': ...},
    {'quant': ..., 'prec': _PREC, 'sample_dtype': 'uint16'}])
def test_version7_bad_header_refused(tmp_path, over):
    # refused for what is wrong with it, not as a version this build does not know
    with pytest.raises(ValueError, match='exception_runs|quant|prec|max_error|float32'):
        container.info(_header(tmp_path, 7, **over))


@pytest.mark.parametrize('version', [2, 3, 4, 5, 6])
def test_other_versions_with_runs_refused(tmp_path, version):
    over = {4: {'sample_dtype': 'uint8', 'max_error': 3, 'quant': ...}, 5: {}, 6: {'quant': ..., 'prec': _PREC}}.get(
        version, {'quant': ...})
    assert container.info(_header(tmp_path, version, exception_runs=..., **over))['version'] == version
    for R in (3, 0, None):
        with pytest.raises(ValueError, match='exception_runs'):
            container.info(_header(tmp_path, version, **dict(over, exception_runs=R)))


def test_plan_region_reads_the_four_run_arrays_whole(tmp_path):
    meta = json.loads(open(_header(tmp_path, 3, quant=..., exception_runs=...), 'rb').read()[container._HEAD.size:])
    plan = container.plan_region(meta, planes=(1, 3))
    assert len(plan['arrays']) == 8
    listed = container.plan_region(dict(meta, quant=_QUANT), planes=(1, 3))
    assert len(listed['arrays']) == 8 + 3 and all(a['shape'] == (12,) for a in listed['arrays'][8:])
    for key, entry in (('quant', _QUANT), ('prec', _PREC)):
        for R in (1, 5, 12):
            rplan = container.plan_region({**meta, key: entry, 'exception_runs': R}, planes=(1, 3))
            assert rplan['arrays'][:8] == plan['arrays'] and len(rplan['arrays']) == 8 + 4
            assert [a['index'] for a in rplan['arrays']] == list(range(12))
            assert {k: v for k, v in rplan.items() if k not in ('arrays', 'tiles_decoded', 'tiles_total')} == \
                {k: v for k, v in plan.items() if k not in ('arrays', 'tiles_decoded', 'tiles_total')}
            for a in rplan['arrays'][8:]:  # read whole, whatever the selection
                assert a['shape'] == (R,) and a['ranges'] == [(0, R, 0)] and a['local_shape'] == (R,)
            assert rplan['tiles_total'] == plan['tiles_total'] + 4
    # without exceptions there is nothing behind the maps, whatever the keyword was
    assert container.plan_region(dict(meta, quant=dict(_QUANT, exceptions=0)), planes=(1, 3))['arrays'] == plan['arrays']


def test_run_extent_check_does_not_wrap():
    """The check that keeps the RUNS kernel's stores inside the array, on host tensors: a start near 2**63
    (whose sum with a length is negative in int64), a negative start, an empty run, a run past the end and
    runs that overlap or step back are all refused; what an encoder writes passes."""
    def check(starts, lengths, numel=1000):
        quant.d_check_runs(torch.tensor(starts, dtype=torch.int64), torch.tensor(lengths, dtype=torch.int64), numel)
    check([0, 5, 990], [5, 3, 10])
    check([], [])
    check([999], [1])
    big = 2 ** 63 - 10
    for starts, lengths in (([big], [100]), ([3, big], [1, 2 ** 32 - 1]), ([2 ** 63 - 1], [1]), ([-1], [1]),
                            ([-2 ** 63], [1]), ([-2 ** 63, 5], [1, 1]), ([0], [0]), ([0], [1001]), ([999], [2]),
                            ([1000], [1]), ([0, 4], [5, 1]), ([10, 9], [1, 1]), ([10, 10], [1, 1]),
                            ([0, 5, 990], [5, 3, 11])):
        with pytest.raises(ValueError):
            check(starts, lengths)
    # the stored form of such a start: d_run_starts sign-extends nothing away, the check sees 2**63 - 10
    u = lambda v: torch.from_numpy(np.array([v], np.uint32))
    starts, lengths, _ = quant.d_run_starts(u(0xfffffff6), u(0x7fffffff), u(100), u(0))
    assert starts.tolist() == [big] and lengths.tolist() == [100]
    with pytest.raises(ValueError):
        quant.d_run_table(u(0xfffffff6), u(0x7fffffff), u(100), u(0), 1000)
