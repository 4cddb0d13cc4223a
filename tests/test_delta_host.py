"""Time series, the host side: every argument error is raised before the device is touched
(these tests run without a GPU), a version-8 header is accepted or refused by its metadata alone, and
``plan_region`` starts a time series' plan at the key frame."""

import json
import os

import numpy as np
import pytest
import torch

import kompressor_amd as kom
from kompressor_amd import _lib, container, delta

import delta_spec as D


def test_exported():
    assert _lib.CODER_DELTA == 13 and container.VERSION_TEMPORAL == 8
    assert {np.dtype(k).name: np.dtype(v).name for k, v in D.SIGNED.items()} == \
        {container._NP_NAME[k]: container._NP_NAME[v] for k, v in delta.SIGNED.items()}
    for t in range(9):
        for K in (None, 1, 2, 3, 8, 9):
            assert delta.is_key(t, K) == D.is_key(t, K)


def test_delta_argument_errors():
    n = np.zeros((3, 4), np.int16)
    for bad in (True, False, 0, -1, 2.0, '2', (2,)):
        with pytest.raises(ValueError):
            delta.encode(n, bad)
        with pytest.raises(ValueError):
            delta.decode(n, np.int16, bad)
    for dt in (np.float32, np.uint32, np.int64):
        with pytest.raises(TypeError):
            delta.encode(np.zeros((3, 4), dt))
        with pytest.raises(TypeError):
            delta.decode(n, dt)
    for dt in (torch.float32, torch.int64, 'float32', 'no-such-dtype', None):
        with pytest.raises(TypeError):
            delta.decode(n, dt)
    with pytest.raises(TypeError):
        delta.decode(n.view(np.uint16), np.uint16)
    with pytest.raises(TypeError):
        delta.decode(n, np.int32)
    with pytest.raises(ValueError):
        delta.encode(np.int16(3))


U16 = np.zeros((3, 5, 5, 5, 1), np.uint16)
F32 = np.zeros((3, 5, 5, 5, 1), np.float32)


@pytest.mark.parametrize('x, kw', [
    (U16, {'key_interval': 2}), (U16, {'key_interval': 0}), (U16, {'temporal': 'Delta'}), (U16, {'temporal': ''}),
    (U16, {'temporal': True}), (U16, {'temporal': 1}), (U16, {'temporal': b'delta'}),
    (U16, {'temporal': 'delta', 'key_interval': 0}), (U16, {'temporal': 'delta', 'key_interval': -3}),
    (U16, {'temporal': 'delta', 'key_interval': True}), (U16, {'temporal': 'delta', 'key_interval': 2.0}),
    (U16, {'temporal': 'delta', 'key_interval': '2'}), (U16, {'temporal': 'delta', 'max_error': 2}),
    (U16, {'temporal': 'delta', 'target_bits': 4.0}), (U16, {'temporal': 'delta', 'target_psnr': 40.0}),
    (U16, {'temporal': 'delta', 'target_ratio': 2.0, 'target_mode': 'near'}),
    (F32, {'temporal': 'delta'}), (F32.view(np.uint32), {'temporal': 'delta'}),
    (F32, {'key_interval': 2, 'abs_error': 1e-3}), (F32, {'key_interval': 2, 'target_bits': 4.0})])
def test_bad_keywords(x, kw, tmp_path):
    pred = kom.MeanPredictor(0, 3)
    with pytest.raises(ValueError):
        container.compress(str(tmp_path / 'x.kmp'), x, pred, levels=1, **kw)
    if not any(k.startswith('target') for k in kw):
        with pytest.raises(ValueError):
            container.compressed_size(x, pred, levels=1, **kw)
    assert not os.listdir(tmp_path)


# ---- headers ------------------------------------------------------------------------------------------------

_QUANT = {'exp': -9, 'dtype': 'int16', 'exceptions': 12}
_PREC = {'bits': 6, 'dtype': 'int32', 'exceptions': 12}
_T16 = {'mode': 'delta', 'key_interval': 2, 'dtype': 'int16'}


def _header(tmp_path, version, **meta_over):
    meta = {'format': 'kompressor_amd', 'ndim': 3, 'padding': 0, 'method': 'rice', 'sample_dtype': 'float32',
            'levels': [{'highres_shape': [5, 5, 5, 5, 1], 'dims': [0, 0, 0]}], 'lowres_shape': [5, 3, 3, 3, 1],
            'predictor': {'kind': 'mean', 'padding': 0, 'ndim': 3}, 'bundle_bytes': 0, 'crc32': 0,
            'quant': _QUANT, 'temporal': _T16}
    meta.update(meta_over)
    meta = {k: v for k, v in meta.items() if v is not ...}
    js = json.dumps(meta, separators=(',', ':')).encode()
    js += b' ' * (-len(js) % 8)
    path = tmp_path / f'v{version}.kmp'
    path.write_bytes(container._HEAD.pack(container.MAGIC, version, 0, len(js)) + js)
    return str(path)


def test_version8_header(tmp_path):
    info = container.info(_header(tmp_path, 8))
    assert info['version'] == 8 and info['temporal'] == 'delta' and info['key_interval'] == 2
    assert info['abs_error'] == 2.0 ** -10 and info['quant_dtype'] == 'int16' and info['shape'] == (5, 5, 5, 5, 1)
    info = container.info(_header(tmp_path, 8, temporal=dict(_T16, key_interval=0)))
    assert info['temporal'] == 'delta' and info['key_interval'] is None
    info = container.info(_header(tmp_path, 8, quant=..., prec=_PREC, temporal=dict(_T16, dtype='int32')))
    assert info['rel_error'] == 2.0 ** -7 and info['key_interval'] == 2
    info = container.info(_header(tmp_path, 8, exception_runs=3))
    assert info['exception_runs'] == 3 and info['temporal'] == 'delta'
    for name, d in (('uint8', 'int8'), ('int8', 'int8'), ('uint16', 'int16'), ('int16', 'int16'), ('int32', 'int32')):
        info = container.info(_header(tmp_path, 8, quant=..., sample_dtype=name, temporal=dict(_T16, dtype=d)))
        assert info['sample_dtype'] == name and info['temporal'] == 'delta' and 'abs_error' not in info
    assert container.level_shapes(_header(tmp_path, 8)) == [(5, 5, 5, 5, 1), (5, 3, 3, 3, 1)]
    # the files of the other versions say nothing of it
    for version, over in ((3, {'quant': ..., 'sample_dtype': 'uint16'}), (5, {}), (7, {'exception_runs': 3})):
        info = container.info(_header(tmp_path, version, temporal=..., **over))
        assert info['version'] == version and 'temporal' not in info and 'key_interval' not in info


@pytest.mark.parametrize('over', [
    {'temporal': ...}, {'temporal': None}, {'temporal': 'delta'}, {'temporal': []}, {'temporal': {}},
    {'temporal': dict(_T16, mode='xor')}, {'temporal': dict(_T16, mode=None)}, {'temporal': dict(_T16, key_interval=-1)},
    {'temporal': dict(_T16, key_interval=True)}, {'temporal': dict(_T16, key_interval=2.0)},
    {'temporal': dict(_T16, key_interval='2')}, {'temporal': dict(_T16, key_interval=None)},
    {'temporal': dict(_T16, dtype='uint16')}, {'temporal': dict(_T16, dtype='float32')}, {'temporal': dict(_T16, dtype=None)},
    {'temporal': dict(_T16, dtype='int32')}, {'temporal': dict(_T16, dtype='int8')},
    {'temporal': {k: v for k, v in _T16.items() if k != 'key_interval'}},
    {'max_error': 0}, {'max_error': 2}, {'max_error': None},
    {'quant': ...}, {'quant': ..., 'sample_dtype': 'uint32'}, {'quant': ..., 'sample_dtype': 'uint8'},
    {'quant': ..., 'sample_dtype': 'int32'}, {'quant': ..., 'sample_dtype': ...},
    {'quant': dict(_QUANT, exp=200)}, {'quant': _QUANT, 'prec': _PREC}, {'exception_runs': 0}, {'exception_runs': 13},
    {'quant': ..., 'sample_dtype': 'uint16', 'exception_runs': 3}])
def test_version8_bad_header_refused(tmp_path, over):
    # refused for what is wrong with it, not as a version this build does not know
    with pytest.raises(ValueError, match='temporal|deltas|max_error|quant|prec|exception_runs'):
        container.info(_header(tmp_path, 8, **over))


@pytest.mark.parametrize('version', [2, 3, 4, 5, 6, 7])
def test_other_versions_with_temporal_refused(tmp_path, version):
    over = {4: {'sample_dtype': 'uint8', 'max_error': 3, 'quant': ...}, 5: {}, 6: {'quant': ..., 'prec': _PREC},
            7: {'exception_runs': 3}}.get(version, {'quant': ..., 'sample_dtype': 'int16'})
    assert container.info(_header(tmp_path, version, temporal=..., **over))['version'] == version
    for t in (_T16, None, {}):
        with pytest.raises(ValueError, match='temporal'):
            container.info(_header(tmp_path, version, **dict(over, temporal=t)))


def test_plan_region_starts_at_the_key_frame(tmp_path):
    meta = json.loads(open(_header(tmp_path, 8), 'rb').read()[container._HEAD.size:])
    plain = {k: v for k, v in meta.items() if k != 'temporal'}
    for K in (None, 1, 2, 3, 5):
        tmeta = dict(meta, temporal=dict(_T16, key_interval=K or 0))
        for a in range(5):
            for b in range(a + 1, 6):
                plan = container.plan_region(tmeta, batch=(a, b), planes=(1, 3))
                a0 = D.frames_read(a, b, K)[0]
                assert plan['batch'] == (a0, b) and plan['frames'] == (a, b)
                want = container.plan_region(plain, batch=(a0, b), planes=(1, 3))
                assert 'frames' not in want and {k: v for k, v in plan.items() if k != 'frames'} == want
    plan = container.plan_region(meta, batch=(3, 4))  # K = 2: no sample of frames 0 - 1
    for ar in plan['arrays'][:8]:
        per = int(np.prod(ar['shape'][1:]))
        assert ar['ranges'] and all(first >= 2 * per and end <= 4 * per for first, end, _ in ar['ranges'])
