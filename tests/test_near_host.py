"""Near-lossless coding, the host side: every argument error is raised before the device is touched
(these tests run without a GPU), and a version-4 header with a bad bound is refused."""

import json
import os

import numpy as np
import pytest
import torch

import kompressor_amd as kom
from kompressor_amd import _lib, _nd, container, near


def test_exported():
    assert kom.near is near
    assert (_lib.CODER_NEAR_U8, _lib.CODER_NEAR_U16) == (4, 5)
    assert _lib.coder_near(_lib.CODER_NEAR_U16, 300) == 5 | (300 << 8)
    assert _nd.CODER_DTYPE[_lib.coder_near(_lib.CODER_NEAR_U8, 7)] == torch.uint8
    assert _nd.CODER_DTYPE[_lib.coder_near(_lib.CODER_NEAR_U16, 7)] == torch.uint16
    with pytest.raises(KeyError):
        _nd.CODER_DTYPE[_lib.CODER_U8 | (1 << 8)]  # a lossless code carries no bound
    assert _nd.coder_fits(near.coder_id(np.int16, 3), torch.int16)
    assert not _nd.coder_fits(near.coder_id(np.int16, 3), torch.uint8)
    assert not _nd.coder_fits(near.coder_id(np.uint8, 3), torch.int32)


@pytest.mark.parametrize('bad', [-1, True, False, 1.0, '1', None, 128, 1 << 20])
def test_coders_bad_max_error(bad):
    with pytest.raises(ValueError):
        near.coders(np.uint8, bad)


def test_coders_bounds_per_dtype():
    for dtype, top in ((np.uint8, 127), (np.int8, 127), (np.uint16, 32767), (np.int16, 32767)):
        assert near.max_error_limit(dtype) == top
        enc, dec = near.coders(dtype, top)
        assert enc._kmp_coder == (near.coder_id(dtype, top), _lib.ENCODE)
        assert dec._kmp_coder == (near.coder_id(dtype, top), _lib.DECODE)
        with pytest.raises(ValueError):
            near.coders(dtype, top + 1)


@pytest.mark.parametrize('dtype', [np.float32, np.int32, np.uint32, torch.float32, 'float32', np.float64])
def test_coders_wide_dtypes(dtype):
    with pytest.raises(TypeError):
        near.coders(dtype, 1)


def test_zero_is_the_lossless_pair():
    assert near.coders(np.uint8, 0) == (kom.utils.encode_values_uint8, kom.utils.decode_values_uint8)
    assert near.coders(torch.uint16, 0) == (kom.utils.encode_values_uint16, kom.utils.decode_values_uint16)
    assert near.coders(np.int8, 0) == (kom.utils.encode_values_int8, kom.utils.decode_values_int8)
    assert near.coders('int16', 0) == (kom.utils.encode_values_int16, kom.utils.decode_values_int16)
    assert near.coder_id(np.uint16, 0) == _lib.CODER_U16


@pytest.mark.parametrize('bad,exc', [(-1, ValueError), (True, ValueError), (2.0, ValueError), (40000, ValueError)])
def test_compress_bad_max_error(tmp_path, bad, exc):
    path = tmp_path / 'x.kmp'
    x = np.zeros((1, 5, 5, 5, 1), np.uint16)
    with pytest.raises(exc):
        container.compress(str(path), x, kom.MeanPredictor(0, 3), levels=1, max_error=bad)
    assert not os.listdir(tmp_path)


@pytest.mark.parametrize('dtype', [np.float32, np.int32, np.uint32])
def test_compress_wide_samples(tmp_path, dtype):
    path = tmp_path / 'x.kmp'
    x = np.zeros((1, 5, 5, 5, 1), dtype)
    with pytest.raises(TypeError):
        container.compress(str(path), x, kom.MeanPredictor(0, 3), levels=1, max_error=1)
    with pytest.raises(TypeError):
        near.encode_pyramid(kom.MeanPredictor(0, 3), x, 1, 1)
    with pytest.raises(TypeError):
        container.save(str(path), x[:, ::2, ::2, ::2], ((), (0, 0, 0)), kom.MeanPredictor(0, 3), max_error=1)
    assert not os.listdir(tmp_path)


def _header(tmp_path, version, **meta_over):
    meta = {'format': 'kompressor_amd', 'ndim': 3, 'padding': 0, 'method': 'rice', 'sample_dtype': 'uint8',
            'levels': [{'highres_shape': [1, 5, 5, 5, 1], 'dims': [0, 0, 0]}], 'lowres_shape': [1, 3, 3, 3, 1],
            'predictor': {'kind': 'mean', 'padding': 0, 'ndim': 3}, 'bundle_bytes': 0, 'crc32': 0}
    meta.update(meta_over)
    meta = {k: v for k, v in meta.items() if v is not ...}
    js = json.dumps(meta, separators=(',', ':')).encode()
    js += b' ' * (-len(js) % 8)
    path = tmp_path / f'v{version}.kmp'
    path.write_bytes(container._HEAD.pack(container.MAGIC, version, 0, len(js)) + js)
    return str(path)


def test_version4_header(tmp_path):
    info = container.info(_header(tmp_path, 4, max_error=3))
    assert info['version'] == 4 and info['max_error'] == 3
    assert 'max_error' not in container.info(_header(tmp_path, 3))


@pytest.mark.parametrize('over', [{'max_error': ...}, {'max_error': 0}, {'max_error': -2}, {'max_error': 128},
                                  {'max_error': 1.5}, {'max_error': True}, {'max_error': '3'},
                                  {'max_error': 40000, 'sample_dtype': 'uint16'},
                                  {'max_error': 1, 'sample_dtype': 'float32'},
                                  {'max_error': 1, 'sample_dtype': 'int32'}])
def test_version4_bad_max_error_refused(tmp_path, over):
    with pytest.raises(ValueError):
        container.info(_header(tmp_path, 4, **over))


def test_older_version_with_a_bound_refused(tmp_path):
    with pytest.raises(ValueError):
        container.info(_header(tmp_path, 3, max_error=2))
    with pytest.raises(ValueError):  # and a version this build does not know
        container.info(_header(tmp_path, 5, max_error=2))
