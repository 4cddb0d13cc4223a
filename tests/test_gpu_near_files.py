"""Near-lossless files: compress / decompress / read_region / save / load / info with ``max_error``,
against the closed loop of tests/near_spec.py bit for bit; the version-4 header; and files with
``max_error=0`` byte-identical to files written without the keyword."""

import os
import struct

import numpy as np
import pytest
import torch

import near_spec as NS

pytestmark = pytest.mark.gpu

DT_IDS = [np.dtype(d).name for d in NS.DTYPES]


def version_of(path):
    with open(path, 'rb') as f:
        return struct.unpack('<4sHHQ', f.read(16))[1]


def data(shape, dtype, seed=0):
    """The noisy field with full-range noise in the second batch entry (or the second half)."""
    x = NS.noisy_field(shape, dtype, seed=seed)
    n = NS.noise(shape, dtype, seed=seed + 1)
    if shape[0] > 1:
        x[1:] = n[1:]
    else:
        x[0, shape[1] // 2:] = n[0, shape[1] // 2:]
    return x


@pytest.mark.parametrize('tile_crc', [False, True], ids=['plain', 'tile_crc'])
@pytest.mark.parametrize('shape,levels,p', [((2, 17, 18, 21, 1), 2, 0), ((2, 29, 37, 1), 3, 1)], ids=['vol', 'img'])
@pytest.mark.parametrize('dtype', NS.DTYPES, ids=DT_IDS)
def test_compress_decompress(kom, tmp_path, dtype, shape, levels, p, tile_crc):
    from kompressor_amd import container
    ndim = len(shape) - 2
    x = data(shape, dtype, seed=3)
    pred = kom.MeanPredictor(p, ndim)
    fn = NS.mean_fn(p, ndim, dtype)
    path = str(tmp_path / 'a.kmp')
    for delta in (2, NS.max_delta(dtype)):
        res = container.compress(path, x, pred, levels=levels, tile_crc=tile_crc, max_error=delta)
        want = NS.encode_pyramid(x, fn, ndim, p, levels, delta)[2][0]
        worst = int(np.abs(want.astype(np.int64) - x.astype(np.int64)).max())
        assert res['max_error'] == delta and res['max_abs_error'] == worst <= delta
        assert res['levels'] == levels and res['bytes'] == os.path.getsize(path)
        assert version_of(path) == 4
        info = container.info(path)
        assert info['version'] == 4 and info['max_error'] == delta and info['shape'] == shape
        assert info['sample_dtype'] == np.dtype(dtype).name and ('tile_crc' in info) == tile_crc
        got = container.decompress(path)
        assert got.dtype == np.dtype(dtype) and np.array_equal(got, want)
        assert container.check(path)['ok']
        assert container.level_shapes(path)[0] == shape


@pytest.mark.parametrize('dtype', [np.uint16, np.int8], ids=['uint16', 'int8'])
def test_max_error_zero_writes_todays_bytes(kom, tmp_path, dtype):
    from kompressor_amd import container
    x = data((2, 17, 18, 21, 1), dtype, seed=5)
    pred = kom.MeanPredictor(0, 3)
    a, b = str(tmp_path / 'a.kmp'), str(tmp_path / 'b.kmp')
    ra = container.compress(a, x, pred, levels=2, tile_crc=True)
    rb = container.compress(b, x, pred, levels=2, tile_crc=True, max_error=0)
    assert open(a, 'rb').read() == open(b, 'rb').read()
    assert version_of(a) == version_of(b) == 3 and 'max_error' not in container.info(b)
    assert ra['bytes'] == rb['bytes'] and rb['max_error'] == 0 and rb['max_abs_error'] == 0
    assert np.array_equal(container.decompress(b), x)
    # save: the same
    lo, enc = kom.volume.encode(pred, kom.near.coders(dtype, 0)[0], x, padding=0)
    container.save(a, lo, enc, pred)
    container.save(b, lo, enc, pred, max_error=0)
    assert open(a, 'rb').read() == open(b, 'rb').read() and version_of(b) == 3


@pytest.mark.parametrize('shape,levels,p', [((2, 21, 26, 23, 1), 2, 0), ((1, 18, 21, 19, 1), 2, 1),
                                            ((2, 33, 41, 1), 2, 0)], ids=['vol-p0', 'vol-p1', 'img'])
@pytest.mark.parametrize('dtype', [np.uint16, np.int16, np.uint8], ids=['uint16', 'int16', 'uint8'])
def test_read_region_equals_the_slices_of_decompress(kom, tmp_path, monkeypatch, dtype, shape, levels, p):
    from kompressor_amd import container
    monkeypatch.setattr(container, '_ROW_CROP_PLANE', 1)  # rows are cropped at every level
    ndim = len(shape) - 2
    x = data(shape, dtype, seed=7)
    path = str(tmp_path / 'r.kmp')
    container.compress(path, x, kom.MeanPredictor(p, ndim), levels=levels, tile_crc=True, max_error=4)
    full = container.decompress(path)
    assert np.abs(full.astype(np.int64) - x.astype(np.int64)).max() <= 4
    for level in range(levels + 1):
        top = full[(slice(None), *[slice(None, None, 2 ** level)] * ndim)]
        sp = top.shape[1:1 + ndim]
        sel = [(s // 3, max(s // 3 + 1, 2 * s // 3)) for s in sp]
        names = ('planes', 'rows', 'cols') if ndim == 3 else ('rows', 'cols')
        picks = [dict(zip(names, sel)), {names[0]: sel[0]}, {names[-1]: (sp[-1] - 1, sp[-1])},
                 {names[-2]: (0, 1), 'batch': (shape[0] - 1, shape[0])}]
        for kw in picks:
            got = container.read_region(path, level=level, **kw)
            assert container.last_timing['partial'] is True
            b0, b1 = kw.get('batch', (0, shape[0]))
            box = [kw.get(n, (0, s)) for n, s in zip(names, sp)]
            want = top[(slice(b0, b1), *[slice(a, b) for a, b in box])]
            assert got.dtype == np.dtype(dtype) and np.array_equal(got, want), (level, kw)


@pytest.mark.parametrize('dtype', [np.uint16, np.int8], ids=['uint16', 'int8'])
@pytest.mark.parametrize('ndim,shape,p', [(3, (2, 9, 10, 13, 1), 1), (2, (2, 13, 18, 1), 0)], ids=['vol', 'img'])
def test_save_load_decompress_one_level(kom, tmp_path, dtype, ndim, shape, p):
    from kompressor_amd import container
    ns = kom.volume if ndim == 3 else kom.image
    x = data(shape, dtype, seed=9)
    delta = 3
    pred = kom.MeanPredictor(p, ndim)
    enc_fn, dec_fn = kom.near.coders(dtype, delta)
    lo, enc = ns.encode(pred, enc_fn, x, padding=p)
    fn = NS.mean_fn(p, ndim, dtype)
    wlo, wmaps, wdims = NS.encode_level(x, fn, ndim, p, delta)
    want = NS.decode_level(wlo, wmaps, wdims, fn, ndim, p, delta)
    path = str(tmp_path / 's.kmp')
    container.save(path, lo, enc, pred, max_error=delta, tile_crc=True)
    assert version_of(path) == 4 and container.info(path)['max_error'] == delta
    lo2, (maps2, dims2), meta = container.load(path, device=False)
    assert meta['max_error'] == delta and tuple(dims2) == wdims and np.array_equal(lo2, wlo)
    assert all(np.array_equal(a, b) for a, b in zip(maps2, wmaps))
    assert np.array_equal(ns.decode(pred, dec_fn, lo2, (maps2, dims2), padding=p), want)
    assert np.array_equal(container.decompress(path), want)
    assert np.array_equal(container.read_region(path, rows=(2, 5)), want[:, 2:5] if ndim == 2 else want[:, :, 2:5])
    with pytest.raises(TypeError):  # lossless maps are not near maps of another width
        container.save(str(tmp_path / 't.kmp'), lo, ([m.astype(np.int32) for m in enc[0]], enc[1]), pred, max_error=delta)
    assert not os.path.exists(tmp_path / 't.kmp')


def test_external_predictions_fn(kom, tmp_path):
    """A near file coded with an opaque predictions_fn decodes when the function is passed, as a
    lossless one does."""
    from kompressor_amd import container
    x = data((2, 9, 10, 13, 1), np.uint16, seed=11)
    builtin = kom.MeanPredictor(0, 3)
    fn = lambda w: builtin(w)  # noqa: E731
    enc_fn, dec_fn = kom.near.coders(np.uint16, 5)
    lo, enc = kom.volume.encode(fn, enc_fn, x, padding=0)
    path = str(tmp_path / 'e.kmp')
    container.save(path, lo, enc, fn, padding=0, ndim=3, max_error=5)
    want = kom.volume.decode(fn, dec_fn, lo, enc, padding=0)
    assert np.abs(want.astype(np.int64) - x.astype(np.int64)).max() <= 5
    assert np.array_equal(container.decompress(path, predictor=fn), want)
    assert np.array_equal(container.read_region(path, planes=(2, 6), predictor=fn), want[:, 2:6])
    with pytest.raises(AssertionError):
        container.decompress(path)


@pytest.mark.parametrize('dtype', [np.float32, np.int32], ids=['float32', 'int32'])
def test_wide_samples_raise_and_leave_no_file(kom, tmp_path, dtype):
    from kompressor_amd import container
    x = np.zeros((1, 9, 9, 9, 1), dtype)
    with pytest.raises(TypeError):
        container.compress(str(tmp_path / 'w.kmp'), x, kom.MeanPredictor(0, 3), levels=1, max_error=1)
    with pytest.raises(TypeError):
        container.compress(str(tmp_path / 'w.kmp'), torch.from_numpy(x).cuda(), kom.MeanPredictor(0, 3), levels=1,
                           max_error=1)
    assert not os.listdir(tmp_path)
    container.compress(str(tmp_path / 'w.kmp'), x, kom.MeanPredictor(0, 3), levels=1)  # lossless: as ever


def test_bits_per_sample_falls(kom, tmp_path):
    from kompressor_amd import container
    x = NS.noisy_field((1, 40, 48, 56, 1), np.uint16, seed=0)
    pred = kom.MeanPredictor(0, 3)
    bits = {d: container.compress(str(tmp_path / f'd{d}.kmp'), x, pred, levels=2, max_error=d)['bits_per_sample']
            for d in (0, 2)}
    print(f'bits per sample: delta 0 {bits[0]:.3f}, delta 2 {bits[2]:.3f}')
    assert bits[2] < bits[0]
