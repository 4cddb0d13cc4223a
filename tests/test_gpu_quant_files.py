"""Error-bounded float32 files: compress(abs_error=...) / decompress / read_region / info / check against
tests/quant_spec.py bit for bit; the version-5 header; and ``abs_error=None`` files byte-identical to
files written without the keyword."""

import os
import struct

import numpy as np
import pytest

import near_spec as NS
import quant_spec as Q
import signed_spec as SS

pytestmark = pytest.mark.gpu

VOL, SMALL, IMG = (1, 20, 24, 33, 1), (2, 9, 10, 13, 1), (2, 21, 18, 1)
ABS_ERROR = 1e-3


def version_of(path):
    with open(path, 'rb') as f:
        return struct.unpack('<4sHHQ', f.read(16))[1]


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def field(shape, variant, seed=0):
    """smooth: quantises to int16 at ABS_ERROR; offset: to int32; exceptions: a NaN block, both infinities,
    NaN payloads and one value past the int32 range; all: nothing that can be quantised."""
    rng = np.random.default_rng(seed)
    x = np.empty(shape, np.float64)
    for b in range(shape[0]):
        x[b, ..., 0] = 3.0 * SS.smooth_field(shape[1:-1], seed + b) + 0.01 * rng.standard_normal(shape[1:-1])
    if variant == 'offset':
        x += 1000.0
    x = x.astype(np.float32)
    if variant == 'exceptions':
        ndim = len(shape) - 2
        x[(0, *[slice(s // 3, s // 3 + 3) for s in shape[1:1 + ndim]])] = np.nan  # a block: even and odd coordinates
        f = x.reshape(-1)
        f[[0, 7, f.size - 1]] = [np.inf, -np.inf, 3e38]
        u32(f)[[f.size // 2, f.size // 2 + 1]] = [0x7fc00001, 0xffc12345]
    if variant == 'all':
        x[...] = np.nan
        x.reshape(-1)[::3] = np.inf
        x.reshape(-1)[1::3] = -np.inf
    return x


def predictor(kom, kind, p, ndim):
    if kind == 'mean':
        return kom.MeanPredictor(p, ndim)
    w, b = NS.linear_weights(p, ndim)
    return kom.LinearPredictor(w, b, p, ndim)


CASES = [(VOL, 'mean', 0, 3, 'smooth'), (VOL, 'mean', 1, 2, 'offset'), (VOL, 'mean', 0, 2, 'exceptions'),
         (VOL, 'linear', 0, 2, 'exceptions'), (VOL, 'mean', 1, 1, 'all'),
         (SMALL, 'mean', 1, 1, 'exceptions'), (SMALL, 'mean', 0, 3, 'all'), (SMALL, 'mean', 0, 2, 'offset'),
         (SMALL, 'linear', 0, 1, 'smooth'),
         (IMG, 'mean', 0, 3, 'exceptions'), (IMG, 'mean', 1, 2, 'smooth'), (IMG, 'linear', 0, 1, 'smooth'),
         (IMG, 'mean', 0, 2, 'all'), (IMG, 'mean', 1, 3, 'offset')]
IDS = [f'{"x".join(map(str, s[1:-1]))}-{k}{p}-L{lv}-{v}' for s, k, p, lv, v in CASES]


def picks(shape, ndim, sp, variant):
    names = ('planes', 'rows', 'cols') if ndim == 3 else ('rows', 'cols')
    third = [(s // 3, max(s // 3 + 1, 2 * s // 3)) for s in sp]
    out = [dict(zip(names, third)), {names[0]: third[0]}, {names[-1]: (sp[-1] - 1, sp[-1])},
           {names[-2]: (0, 1), 'batch': (shape[0] - 1, shape[0])}, {},
           {names[0]: (sp[0] - 1, sp[0]), names[-1]: (0, 1)}]
    return names, out


@pytest.mark.parametrize('shape,kind,p,levels,variant', CASES, ids=IDS)
def test_files(kom, tmp_path, monkeypatch, shape, kind, p, levels, variant):
    from kompressor_amd import container
    monkeypatch.setattr(container, '_ROW_CROP_PLANE', 1)  # rows are cropped at every level
    ndim = len(shape) - 2
    x = field(shape, variant, seed=len(shape) + p)
    e, eps = Q.exponent(ABS_ERROR), Q.effective(ABS_ERROR)
    n_want, exc_want = Q.quantise(x, e)
    want = Q.restore(n_want, e, exc_want)
    E = 0 if exc_want is None else exc_want[0].size
    assert n_want.dtype == (np.int32 if variant == 'offset' else np.int16)
    assert {'smooth': E == 0, 'offset': E == 0, 'exceptions': 0 < E < x.size, 'all': E == x.size}[variant]
    pred = predictor(kom, kind, p, ndim)
    path = str(tmp_path / 'q.kmp')
    res = container.compress(path, x, pred, levels=levels, tile_crc=True, abs_error=ABS_ERROR)
    ok = np.ones(x.size, bool)
    if E:
        ok[exc_want[0]] = False
    worst = float(np.abs(want.reshape(-1)[ok].astype(np.float64) - x.reshape(-1)[ok].astype(np.float64)).max(initial=0.0))
    assert worst <= eps
    assert res['abs_error'] == eps and res['abs_error_asked'] == ABS_ERROR and res['exceptions'] == E
    assert isinstance(res['max_abs_error'], float) and res['max_abs_error'] == worst
    assert res['quant_dtype'] == n_want.dtype.name and res['levels'] == levels and res['bytes'] == os.path.getsize(path)
    assert version_of(path) == 5
    info = container.info(path)
    assert info['version'] == 5 and info['shape'] == shape and info['sample_dtype'] == 'float32'
    assert info['abs_error'] == eps and info['quant_dtype'] == n_want.dtype.name and info['exceptions'] == E
    assert info['levels'] == levels and 'tile_crc' in info and 'max_error' not in info
    shapes = container.level_shapes(path)
    assert shapes[0] == shape and len(shapes) == levels + 1
    full = container.decompress(path)
    assert full.dtype == np.float32 and full.shape == shape and np.array_equal(u32(full), u32(want))
    assert container.check(path)['ok'] and container.check(path)['tile_crc']['bad'] == []
    saw_exception = saw_none = False
    for level in range(levels + 1):
        top = want[(slice(None), *[slice(None, None, 2 ** level)] * ndim)]
        assert shapes[level] == top.shape
        sp = top.shape[1:1 + ndim]
        names, sel = picks(shape, ndim, sp, variant)
        for kw in sel:
            got = container.read_region(path, level=level, **kw)
            assert container.last_timing['partial'] is True and container.last_timing['tile_crc'] is True
            b0, b1 = kw.get('batch', (0, shape[0]))
            box = [kw.get(nm, (0, s)) for nm, s in zip(names, sp)]
            cut = top[(slice(b0, b1), *[slice(a, b) for a, b in box])]
            assert got.dtype == np.float32 and got.shape == cut.shape and np.array_equal(u32(got), u32(cut)), (level, kw)
            saw_exception |= bool((~np.isfinite(cut)).any())
            saw_none |= bool(np.isfinite(cut).all())
    if variant == 'exceptions':
        assert saw_exception and saw_none  # boxes that contain exceptions, and boxes that miss them all


@pytest.mark.parametrize('variant', ['smooth', 'exceptions'])
def test_without_tile_crc_and_device_input(kom, tmp_path, variant):
    import torch
    from kompressor_amd import container
    x = field(SMALL, variant, seed=5)
    e = Q.exponent(1e-2)
    n, exc = Q.quantise(x, e)
    want = Q.restore(n, e, exc)
    path = str(tmp_path / 'd.kmp')
    res = container.compress(path, torch.from_numpy(x).cuda(), kom.MeanPredictor(0, 3), abs_error=1e-2)
    assert res['abs_error'] == Q.effective(1e-2) and 'tile_crc' not in container.info(path)
    got = container.decompress(path, as_numpy=False)
    assert got.is_cuda and got.dtype == torch.float32 and np.array_equal(u32(got.cpu().numpy()), u32(want))
    assert np.array_equal(u32(container.read_region(path, planes=(2, 5), cols=(3, 9))), u32(want[:, 2:5, :, 3:9]))
    assert container.last_timing['tile_crc'] is False
    assert container.check(path) == {'ok': True, 'crc32': True, 'tile_crc': None}
    planes = str(tmp_path / 'p.kmp')  # a bundle without tiles: read whole, then sliced
    container.compress(planes, x, kom.MeanPredictor(0, 3), levels=2, method='planes', abs_error=1e-2)
    assert np.array_equal(u32(container.decompress(planes)), u32(want))
    assert np.array_equal(u32(container.read_region(planes, rows=(1, 4), level=1)), u32(want[:, ::2, ::2, ::2][:, :, 1:4]))
    assert container.last_timing['partial'] is False


def _damage(path, out, at):
    raw = bytearray(open(path, 'rb').read())
    raw[at] ^= 0x10
    open(out, 'wb').write(bytes(raw))
    return out


def test_check_names_a_damaged_tile(kom, tmp_path):
    from kompressor_amd import container, packing
    x = field(VOL, 'exceptions', seed=9)
    path = str(tmp_path / 'c.kmp')
    container.compress(path, x, kom.MeanPredictor(0, 3), levels=2, tile_crc=True, abs_error=ABS_ERROR)
    raw = open(path, 'rb').read()
    mlen = struct.unpack('<4sHHQ', raw[:16])[3]
    base = 16 + mlen
    count = packing._RHEAD.unpack(raw[base:base + packing._RHEAD.size])[2]
    plan = packing._rice_dec_plan(None, raw[base:base + packing._RHEAD.size + packing._RREC.size * count])
    assert count == 1 + 7 * 2 + 3 and plan['shapes'][-1] == plan['shapes'][-2] == plan['shapes'][-3]
    E = container.info(path)['exceptions']
    assert plan['shapes'][-1] == (E,) and 0 < E < 16384
    # a payload byte of the first map, and one of the exceptions' bits (the last array): both are named
    for which, a in (('map', 1), ('bits', count - 1)):
        bad = _damage(path, str(tmp_path / f'{which}.kmp'), base + plan['poff'] + 4 * plan['spans'][a][0] + 1)
        got = container.check(bad)
        assert got['ok'] is False and got['crc32'] is False and got['tile_crc']['bad'] == [(a, 0)]
        with pytest.raises(ValueError):
            container.decompress(bad)
    with pytest.raises(ValueError, match='tile CRC mismatch'):  # the exception arrays are read whole and checked
        container.read_region(str(tmp_path / 'bits.kmp'), planes=(0, 2))


@pytest.mark.parametrize('dtype', [np.float32, np.uint16], ids=['float32', 'uint16'])
def test_abs_error_none_writes_todays_bytes(kom, tmp_path, dtype):
    from kompressor_amd import container
    x = field(SMALL, 'exceptions', seed=3) if dtype == np.float32 else NS.noisy_field(SMALL, np.uint16, seed=3)
    pred = kom.MeanPredictor(0, 3)
    a, b = str(tmp_path / 'a.kmp'), str(tmp_path / 'b.kmp')
    ra = container.compress(a, x, pred, levels=2, tile_crc=True)
    rb = container.compress(b, x, pred, levels=2, tile_crc=True, abs_error=None)
    assert open(a, 'rb').read() == open(b, 'rb').read() and version_of(b) == 3 and ra == rb
    assert not {'abs_error', 'quant_dtype', 'exceptions'} & set(container.info(b))
    assert np.array_equal(container.decompress(b).view(np.uint32 if dtype == np.float32 else dtype),
                          x.view(np.uint32 if dtype == np.float32 else dtype))  # lossless float32: bit for bit


def test_a_broken_bound_writes_nothing(kom, tmp_path, monkeypatch):
    from kompressor_amd import container
    x = field(SMALL, 'smooth', seed=1)
    monkeypatch.setattr(container, '_quant_max_error', lambda *a: 1.0)
    with pytest.raises(RuntimeError):
        container.compress(str(tmp_path / 'x.kmp'), x, kom.MeanPredictor(0, 3), abs_error=1e-3)
    assert not os.listdir(tmp_path)


def test_file_size_on_the_spec_field(kom, tmp_path):
    from kompressor_amd import container
    x = Q.spec_field()
    pred = kom.MeanPredictor(0, 3)
    bits = {a: container.compress(str(tmp_path / 'f.kmp'), x, pred, levels=2, abs_error=a)['bits_per_sample']
            for a in (None, 1e-1, 1e-2, 1e-3, 1e-4)}
    print('bits per sample:', {str(a): round(v, 3) for a, v in bits.items()})
    assert bits[1e-2] < 8.0
    assert bits[1e-1] < bits[1e-2] < bits[1e-3] < bits[1e-4] < bits[None]
