"""Error-bounded float32 coding, the host side: every argument error is raised before the device is
touched (these tests run without a GPU), and a version-5 header is accepted or refused by its
metadata alone."""

import json
import math
import os

import numpy as np
import pytest
import torch

import kompressor_amd as kom
from kompressor_amd import _lib, _nd, container, quant

import quant_spec as Q


def test_exported():
    assert kom.quant is quant
    assert (_lib.CODER_QUANT_I16, _lib.CODER_QUANT_I32) == (6, 7)
    assert _nd.CODER_DTYPE[_lib.CODER_QUANT_I16] == torch.int16
    assert _nd.CODER_DTYPE[_lib.CODER_QUANT_I32] == torch.int32
    assert _nd.CODER_DTYPE[_lib.coder_quant(_lib.CODER_QUANT_I16, -10)] == torch.int16
    assert _nd.CODER_DTYPE[_lib.coder_quant(_lib.CODER_QUANT_I32, 127)] == torch.int32
    assert container.VERSION_QUANT == 5


def test_coder_quant_bit_layout():
    assert _lib.coder_quant(6, -126) == 6 | (1 << 8)
    assert _lib.coder_quant(7, 0) == 7 | (127 << 8)
    assert _lib.coder_quant(7, 127) == 7 | (254 << 8)
    for e in (-126, -1, 0, 5, 127):
        c = _lib.coder_quant(_lib.CODER_QUANT_I16, e)
        assert _lib.coder_code(c) == 6 and (c >> 8) - 127 == e and 0 < c < 2 ** 31


def test_exponent_is_the_specs():
    for a in (1e-4, 1e-3, 1e-2, 1e-1, 0.5, 1, 3, 2.0 ** -127, 2.0 ** 126, np.float32(0.25), np.int64(7)):
        assert quant.exponent(a) == Q.exponent(a) and quant.effective(a) == Q.effective(a)
    assert (quant.E_MIN, quant.E_MAX) == (Q.E_MIN, Q.E_MAX)


BAD_BOUNDS = [True, False, '1e-3', None, math.nan, math.inf, -math.inf, 0, 0.0, -1e-3, 2.0 ** -128, 2.0 ** 127, 1e300,
              10 ** 400]


@pytest.mark.parametrize('bad', BAD_BOUNDS)
def test_bad_abs_error(bad, tmp_path):
    x = np.zeros((1, 5, 5, 5, 1), np.float32)
    with pytest.raises(ValueError):
        quant.exponent(bad)
    with pytest.raises(ValueError):
        quant.effective(bad)
    with pytest.raises(ValueError):
        quant.quantise(x, bad)
    if bad is not None:  # compress(abs_error=None) is the lossless file
        with pytest.raises(ValueError):
            container.compress(str(tmp_path / 'x.kmp'), x, kom.MeanPredictor(0, 3), levels=1, abs_error=bad)
    assert not os.listdir(tmp_path)


@pytest.mark.parametrize('dtype', [np.float64, np.int16, np.int32, np.uint32, np.uint16])
def test_not_float32(dtype, tmp_path):
    x = np.zeros((1, 5, 5, 5, 1), dtype)
    with pytest.raises(TypeError):
        quant.quantise(x, 1e-3)
    with pytest.raises(TypeError):
        quant.quantise(torch.zeros(4, dtype=torch.float64), 1e-3)
    with pytest.raises(TypeError):
        container.compress(str(tmp_path / 'x.kmp'), x, kom.MeanPredictor(0, 3), levels=1, abs_error=1e-3)
    assert not os.listdir(tmp_path)


def test_restore_arguments():
    with pytest.raises(TypeError):
        quant.restore(np.zeros(4, np.float32), 0)
    with pytest.raises(TypeError):
        quant.restore(np.zeros(4, np.uint16), 0)
    for bad in (-127, 128, 1.0, True, None, '0'):
        with pytest.raises(ValueError):
            quant.restore(np.zeros(4, np.int16), bad)
    with pytest.raises(TypeError):
        quant.restore(np.zeros(4, np.int16), 0, (np.zeros(1, np.int32), np.zeros(1, np.uint32)))
    with pytest.raises(TypeError):
        quant.restore(np.zeros(4, np.int16), 0, (np.zeros(1, np.int64), np.zeros(1, np.float32)))


def test_abs_error_excludes_max_error(tmp_path):
    for x in (np.zeros((1, 5, 5, 5, 1), np.float32), np.zeros((1, 5, 5, 5, 1), np.uint16)):
        with pytest.raises(ValueError):
            container.compress(str(tmp_path / 'x.kmp'), x, kom.MeanPredictor(0, 3), levels=1, max_error=1, abs_error=1e-3)
    assert not os.listdir(tmp_path)


def _header(tmp_path, version, **meta_over):
    meta = {'format': 'kompressor_amd', 'ndim': 3, 'padding': 0, 'method': 'rice', 'sample_dtype': 'float32',
            'levels': [{'highres_shape': [1, 5, 5, 5, 1], 'dims': [0, 0, 0]}], 'lowres_shape': [1, 3, 3, 3, 1],
            'predictor': {'kind': 'mean', 'padding': 0, 'ndim': 3}, 'bundle_bytes': 0, 'crc32': 0,
            'quant': {'exp': -9, 'dtype': 'int16', 'exceptions': 0}}
    meta.update(meta_over)
    meta = {k: v for k, v in meta.items() if v is not ...}
    js = json.dumps(meta, separators=(',', ':')).encode()
    js += b' ' * (-len(js) % 8)
    path = tmp_path / f'v{version}.kmp'
    path.write_bytes(container._HEAD.pack(container.MAGIC, version, 0, len(js)) + js)
    return str(path)


def test_version5_header(tmp_path):
    info = container.info(_header(tmp_path, 5))
    assert info['version'] == 5 and info['sample_dtype'] == 'float32' and info['shape'] == (1, 5, 5, 5, 1)
    assert info['abs_error'] == 2.0 ** -10 and info['quant_dtype'] == 'int16' and info['exceptions'] == 0
    assert 'max_error' not in info
    info = container.info(_header(tmp_path, 5, quant={'exp': 127, 'dtype': 'int32', 'exceptions': 12}))
    assert info['abs_error'] == 2.0 ** 126 and info['quant_dtype'] == 'int32' and info['exceptions'] == 12
    assert container.info(_header(tmp_path, 5, quant={'exp': -126, 'dtype': 'int16', 'exceptions': 0}))['abs_error'] == \
        2.0 ** -127
    assert container.level_shapes(_header(tmp_path, 5)) == [(1, 5, 5, 5, 1), (1, 3, 3, 3, 1)]
    plain = container.info(_header(tmp_path, 3, quant=...))
    assert not {'abs_error', 'quant_dtype', 'exceptions'} & set(plain)


def _q(**over):
    q = {'exp': -9, 'dtype': 'int16', 'exceptions': 0}
    q.update(over)
    return {k: v for k, v in q.items() if v is not ...}


@pytest.mark.parametrize('over', [
    {'quant': ...}, {'quant': None}, {'quant': 7}, {'quant': []}, {'quant': {}},
    {'quant': _q(exp=-127)}, {'quant': _q(exp=128)}, {'quant': _q(exp=1.0)}, {'quant': _q(exp=True)},
    {'quant': _q(exp='0')}, {'quant': _q(exp=...)},
    {'quant': _q(dtype='int8')}, {'quant': _q(dtype='float32')}, {'quant': _q(dtype=2)}, {'quant': _q(dtype=...)},
    {'quant': _q(exceptions=-1)}, {'quant': _q(exceptions=1.5)}, {'quant': _q(exceptions=True)},
    {'quant': _q(exceptions='3')}, {'quant': _q(exceptions=...)},
    {'sample_dtype': 'int16'}, {'sample_dtype': 'uint32'}, {'sample_dtype': ...},
    {'max_error': 0}, {'max_error': 2}, {'max_error': None}])
def test_version5_bad_header_refused(tmp_path, over):
    with pytest.raises(ValueError):
        container.info(_header(tmp_path, 5, **over))


@pytest.mark.parametrize('version', [2, 3, 4])
def test_older_version_with_quant_refused(tmp_path, version):
    over = {'sample_dtype': 'uint8', 'max_error': 3} if version == 4 else {}
    with pytest.raises(ValueError):
        container.info(_header(tmp_path, version, **over))
    assert container.info(_header(tmp_path, version, quant=..., **over))['version'] == version
    with pytest.raises(ValueError):  # and a version this build does not know
        container.info(_header(tmp_path, 6))


def test_plan_region_unchanged_without_quant_and_extended_with_it(tmp_path):
    meta = json.loads(open(_header(tmp_path, 3, quant=...), 'rb').read()[container._HEAD.size:])
    plan = container.plan_region(meta, planes=(1, 3))
    assert len(plan['arrays']) == 8 and [a['index'] for a in plan['arrays']] == list(range(8))
    for E, extra in ((0, 0), (5, 3)):
        qmeta = dict(meta, quant={'exp': 0, 'dtype': 'int16', 'exceptions': E})
        qplan = container.plan_region(qmeta, planes=(1, 3))
        assert qplan['arrays'][:8] == plan['arrays'] and len(qplan['arrays']) == 8 + extra
        assert {k: v for k, v in qplan.items() if k not in ('arrays', 'tiles_decoded', 'tiles_total')} == \
            {k: v for k, v in plan.items() if k not in ('arrays', 'tiles_decoded', 'tiles_total')}
        for a in qplan['arrays'][8:]:  # read whole, whatever the selection
            assert a['shape'] == (E,) and a['ranges'] == [(0, E, 0)] and a['local_shape'] == (E,)
        assert qplan['tiles_total'] == plan['tiles_total'] + extra
