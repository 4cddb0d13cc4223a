"""Relative-error float32 coding, the host side: every argument error is raised before the device is
touched (these tests run without a GPU), and a version-6 header is accepted or refused by its
metadata alone."""

import json
import math
import os

import numpy as np
import pytest
import torch

import kompressor_amd as kom
from kompressor_amd import _lib, _nd, container, quant

import prec_spec as P


def test_exported():
    assert (_lib.CODER_PREC_I16, _lib.CODER_PREC_I32) == (8, 9)
    assert _lib.coder_prec(8, 0) == 8 | 1 << 8
    assert _lib.coder_prec(9, 22) == 9 | 23 << 8
    for m in (0, 7, 8, 22):
        c = _lib.coder_prec(_lib.CODER_PREC_I32, m)
        assert _lib.coder_code(c) == 9 and (c >> 8) - 1 == m and 0 < c < 2 ** 31
    assert _nd.CODER_DTYPE[_lib.CODER_PREC_I16] == torch.int16
    assert _nd.CODER_DTYPE[_lib.CODER_PREC_I32] == torch.int32
    assert _nd.CODER_DTYPE[_lib.coder_prec(_lib.CODER_PREC_I16, 3)] == torch.int16
    assert _nd.CODER_DTYPE[_lib.coder_prec(_lib.CODER_PREC_I32, 22)] == torch.int32
    for dt in (torch.int16, torch.int32, torch.float32):  # no codec coder
        assert not _nd.coder_fits(_lib.coder_prec(_lib.CODER_PREC_I16, 3), dt)
        assert not _nd.coder_fits(_lib.CODER_PREC_I32, dt)
    assert not _nd.is_near(_lib.coder_prec(_lib.CODER_PREC_I16, 5))
    assert container.VERSION_PREC == 6 and container.VERSION_QUANT == 5
    assert (quant.M_MIN, quant.M_MAX) == (P.M_MIN, P.M_MAX)


def test_mantissa_bits_is_the_specs():
    for r in (0.5, 0.3, 1e-1, 1e-2, 1e-3, 1e-6, 2.0 ** -23, math.nextafter(1.0, 0.0), np.float32(0.25), np.float64(1e-4)):
        assert quant.mantissa_bits(r) == P.mantissa_bits(r) and quant.effective_rel(r) == P.effective_rel(r)
    assert quant.mantissa_bits(1e-2) == 6 and quant.effective_rel(1e-2) == 2.0 ** -7


BAD_BOUNDS = [True, False, '1e-3', b'1', None, math.nan, math.inf, -math.inf, 0, 0.0, -1e-3, 1, 1.0, 2.5, 2.0 ** -24,
              math.nextafter(2.0 ** -23, 0.0), 1e300, 10 ** 400]


@pytest.mark.parametrize('bad', BAD_BOUNDS)
def test_bad_rel_error(bad, tmp_path):
    x = np.zeros((1, 5, 5, 5, 1), np.float32)
    with pytest.raises(ValueError):
        quant.mantissa_bits(bad)
    with pytest.raises(ValueError):
        quant.effective_rel(bad)
    with pytest.raises(ValueError):
        quant.quantise_rel(x, bad)
    if bad is not None:  # compress(rel_error=None) is the lossless file
        with pytest.raises(ValueError):
            container.compress(str(tmp_path / 'x.kmp'), x, kom.MeanPredictor(0, 3), levels=1, rel_error=bad)
    assert not os.listdir(tmp_path)


@pytest.mark.parametrize('dtype', [np.float64, np.float16, np.int16, np.int32, np.uint32, np.uint16])
def test_not_float32(dtype, tmp_path):
    x = np.zeros((1, 5, 5, 5, 1), dtype)
    with pytest.raises(TypeError):
        quant.quantise_rel(x, 1e-3)
    with pytest.raises(TypeError):
        quant.quantise_rel(torch.zeros(4, dtype=torch.float64), 1e-3)
    with pytest.raises(TypeError):
        container.compress(str(tmp_path / 'x.kmp'), x, kom.MeanPredictor(0, 3), levels=1, rel_error=1e-3)
    assert not os.listdir(tmp_path)


def test_restore_rel_arguments():
    with pytest.raises(TypeError):
        quant.restore_rel(np.zeros(4, np.float32), 6)
    with pytest.raises(TypeError):
        quant.restore_rel(np.zeros(4, np.uint16), 6)
    with pytest.raises(TypeError):
        quant.restore_rel(np.zeros(4, np.int64), 6)
    for bad in (-1, 23, 100, 1.0, True, None, '6'):
        with pytest.raises(ValueError):
            quant.restore_rel(np.zeros(4, np.int16), bad)
    with pytest.raises(TypeError):
        quant.restore_rel(np.zeros(4, np.int16), 6, (np.zeros(1, np.int32), np.zeros(1, np.uint32)))
    with pytest.raises(TypeError):
        quant.restore_rel(np.zeros(4, np.int16), 6, (np.zeros(1, np.int64), np.zeros(1, np.float32)))


def test_bounds_exclude_each_other(tmp_path):
    pred = kom.MeanPredictor(0, 3)
    for x in (np.zeros((1, 5, 5, 5, 1), np.float32), np.zeros((1, 5, 5, 5, 1), np.uint16)):
        for kw in ({'max_error': 1}, {'abs_error': 1e-3}, {'max_error': 1, 'abs_error': 1e-3}):
            with pytest.raises(ValueError):
                container.compress(str(tmp_path / 'x.kmp'), x, pred, levels=1, rel_error=1e-3, **kw)
    assert not os.listdir(tmp_path)


def _header(tmp_path, version, **meta_over):
    meta = {'format': 'kompressor_amd', 'ndim': 3, 'padding': 0, 'method': 'rice', 'sample_dtype': 'float32',
            'levels': [{'highres_shape': [1, 5, 5, 5, 1], 'dims': [0, 0, 0]}], 'lowres_shape': [1, 3, 3, 3, 1],
            'predictor': {'kind': 'mean', 'padding': 0, 'ndim': 3}, 'bundle_bytes': 0, 'crc32': 0,
            'prec': {'bits': 6, 'dtype': 'int16', 'exceptions': 0}}
    meta.update(meta_over)
    meta = {k: v for k, v in meta.items() if v is not ...}
    js = json.dumps(meta, separators=(',', ':')).encode()
    js += b' ' * (-len(js) % 8)
    path = tmp_path / f'v{version}.kmp'
    path.write_bytes(container._HEAD.pack(container.MAGIC, version, 0, len(js)) + js)
    return str(path)


def test_version6_header(tmp_path):
    info = container.info(_header(tmp_path, 6))
    assert info['version'] == 6 and info['sample_dtype'] == 'float32' and info['shape'] == (1, 5, 5, 5, 1)
    assert info['rel_error'] == 2.0 ** -7 and info['quant_dtype'] == 'int16' and info['exceptions'] == 0
    assert 'max_error' not in info and 'abs_error' not in info
    info = container.info(_header(tmp_path, 6, prec={'bits': 22, 'dtype': 'int32', 'exceptions': 12}))
    assert info['rel_error'] == 2.0 ** -23 and info['quant_dtype'] == 'int32' and info['exceptions'] == 12
    assert container.info(_header(tmp_path, 6, prec={'bits': 0, 'dtype': 'int16', 'exceptions': 0}))['rel_error'] == 0.5
    assert container.level_shapes(_header(tmp_path, 6)) == [(1, 5, 5, 5, 1), (1, 3, 3, 3, 1)]
    plain = container.info(_header(tmp_path, 3, prec=...))
    assert not {'rel_error', 'abs_error', 'quant_dtype', 'exceptions'} & set(plain)


def _p(**over):
    p = {'bits': 6, 'dtype': 'int16', 'exceptions': 0}
    p.update(over)
    return {k: v for k, v in p.items() if v is not ...}


_QUANT = {'exp': -9, 'dtype': 'int16', 'exceptions': 0}


@pytest.mark.parametrize('over', [
    {'prec': ...}, {'prec': None}, {'prec': 7}, {'prec': []}, {'prec': {}},
    {'prec': _p(bits=-1)}, {'prec': _p(bits=23)}, {'prec': _p(bits=6.0)}, {'prec': _p(bits=True)},
    {'prec': _p(bits='6')}, {'prec': _p(bits=...)},
    {'prec': _p(dtype='int8')}, {'prec': _p(dtype='float32')}, {'prec': _p(dtype=2)}, {'prec': _p(dtype=...)},
    {'prec': _p(exceptions=-1)}, {'prec': _p(exceptions=1.5)}, {'prec': _p(exceptions=True)},
    {'prec': _p(exceptions='3')}, {'prec': _p(exceptions=...)},
    {'sample_dtype': 'int16'}, {'sample_dtype': 'uint32'}, {'sample_dtype': ...},
    {'max_error': 0}, {'max_error': 2}, {'max_error': None},
    {'quant': _QUANT}, {'quant': None}, {'quant': _QUANT, 'prec': ...}])
def test_version6_bad_header_refused(tmp_path, over):
    with pytest.raises(ValueError):
        container.info(_header(tmp_path, 6, **over))


@pytest.mark.parametrize('version', [2, 3, 4, 5])
def test_other_version_with_prec_refused(tmp_path, version):
    over = {4: {'sample_dtype': 'uint8', 'max_error': 3}, 5: {'quant': _QUANT}}.get(version, {})
    with pytest.raises(ValueError):
        container.info(_header(tmp_path, version, **over))
    assert container.info(_header(tmp_path, version, prec=..., **over))['version'] == version
    with pytest.raises(ValueError):  # and a version this build does not know
        container.info(_header(tmp_path, 7))
    with pytest.raises(ValueError):
        container.info(_header(tmp_path, 7, prec=...))


def test_plan_region_unchanged_without_prec_and_extended_with_it(tmp_path):
    meta = json.loads(open(_header(tmp_path, 3, prec=...), 'rb').read()[container._HEAD.size:])
    plan = container.plan_region(meta, planes=(1, 3))
    assert len(plan['arrays']) == 8 and [a['index'] for a in plan['arrays']] == list(range(8))
    for E, extra in ((0, 0), (5, 3)):
        pmeta = dict(meta, prec={'bits': 6, 'dtype': 'int16', 'exceptions': E})
        pplan = container.plan_region(pmeta, planes=(1, 3))
        assert pplan['arrays'][:8] == plan['arrays'] and len(pplan['arrays']) == 8 + extra
        assert [a['index'] for a in pplan['arrays']] == list(range(8 + extra))
        assert {k: v for k, v in pplan.items() if k not in ('arrays', 'tiles_decoded', 'tiles_total')} == \
            {k: v for k, v in plan.items() if k not in ('arrays', 'tiles_decoded', 'tiles_total')}
        for a in pplan['arrays'][8:]:  # read whole, whatever the selection
            assert a['shape'] == (E,) and a['ranges'] == [(0, E, 0)] and a['local_shape'] == (E,)
        assert pplan['tiles_total'] == plan['tiles_total'] + extra
