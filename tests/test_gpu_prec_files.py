"""Relative-error float32 files: compress(rel_error=...) / decompress / read_region / info / check against
tests/prec_spec.py bit for bit; the version-6 header; and files written with all three bounds ``None``
byte-identical to files written without the keyword.

The shapes are the smallest with more than one batch entry, odd and even extents after halving, and
three levels; the fitted LinearPredictor is fitted on the int16 array, so it runs at m = 6."""

import os
import struct

import numpy as np
import pytest

import prec_spec as P
import signed_spec as SS

pytestmark = pytest.mark.gpu

VOL, IMG = (2, 7, 9, 11, 1), (2, 9, 11, 1)
REL = {6: 1e-2, 10: 2.0 ** -11}  # m = 6: int16 whatever the data; m = 10: int32 on this field


def version_of(path):
    with open(path, 'rb') as f:
        return struct.unpack('<4sHHQ', f.read(16))[1]


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def planted(shape):
    """Coordinates of planted exceptions: a node of every level (all zero; multiples of 4), a node of
    level 1 alone (twice an odd number), non-nodes (odd), in both batch entries."""
    ndim = len(shape) - 2
    sp = shape[1:1 + ndim]
    return [(0, *[0] * ndim, 0), (1, *[4 * ((s - 1) // 4) for s in sp], 0), (0, *[4] * ndim, 0), (0, *[2] * ndim, 0),
            (1, *[2 * (((s - 1) // 2) | 1) if 2 * (((s - 1) // 2) | 1) < s else 2 for s in sp], 0),
            (1, *[1] * ndim, 0), (0, *[s - 2 for s in sp], 0), (0, 3, *[4] * (ndim - 1), 0)]


RAW = [0x7fc00000, 0x7f800000, 0xff800000, 0x7f7fffff, 0xffc12345, 0x7f800001, 0xff7fffff, 0x7fffffff]


def field(shape, exceptions, seed=0):
    """Positive and negative values over about six decades with 5 % multiplicative noise; with
    ``exceptions``, NaNs (payloads, both signs), both infinities and +-FLT_MAX at ``planted(shape)``."""
    rng = np.random.default_rng(seed)
    x = np.empty(shape, np.float64)
    for b in range(shape[0]):
        s = SS.smooth_field(shape[1:-1], seed + b)
        x[b, ..., 0] = np.sign(s + 0.3) * 10.0 ** (3.0 * s) * (1.0 + 0.05 * rng.standard_normal(shape[1:-1]))
    x = x.astype(np.float32)
    if exceptions:
        for at, bits in zip(planted(shape), RAW):
            u32(x)[at] = bits  # x is contiguous: the view writes through
    return x


def predictor(kom, kind, p, ndim, n):
    if kind == 'mean':
        return kom.MeanPredictor(p, ndim)
    assert n.dtype == np.int16
    return kom.LinearPredictor.fit(n, padding=p, ndim=ndim)


CASES = [(VOL, 'mean', 0, 3, 6, True), (VOL, 'mean', 0, 2, 10, True), (VOL, 'mean', 1, 1, 10, False),
         (VOL, 'mean', 1, 2, 6, True), (VOL, 'fit', 0, 2, 6, True), (VOL, 'mean', 0, 1, 6, False),
         (IMG, 'mean', 0, 3, 10, True), (IMG, 'mean', 1, 2, 6, False), (IMG, 'fit', 0, 1, 6, True),
         (IMG, 'mean', 0, 2, 6, True), (IMG, 'mean', 1, 3, 10, True)]
IDS = [f'{"x".join(map(str, s[1:-1]))}-{k}{p}-L{lv}-m{m}-{"exc" if e else "clean"}' for s, k, p, lv, m, e in CASES]


def picks(shape, ndim, sp):
    names = ('planes', 'rows', 'cols') if ndim == 3 else ('rows', 'cols')
    third = [(s // 3, max(s // 3 + 1, 2 * s // 3)) for s in sp]
    out = [dict(zip(names, third)), {names[0]: third[0]}, {names[-1]: (sp[-1] - 1, sp[-1])},
           {names[-2]: (0, 1), 'batch': (shape[0] - 1, shape[0])}, {},
           {names[0]: (sp[0] - 1, sp[0]), names[-1]: (0, 1)}]
    return names, out


def test_planted_coordinates_cover_nodes_and_non_nodes():
    for shape in (VOL, IMG):
        ndim = len(shape) - 2
        at = planted(shape)
        assert len(set(at)) == len(at) == len(RAW)
        assert all(0 <= c < s for a in at for c, s in zip(a, shape))
        node = {k: [a for a in at if all(c % 2 ** k == 0 for c in a[1:1 + ndim])] for k in (1, 2, 3)}
        assert len(node[1]) >= 4 and 2 <= len(node[2]) < len(node[1]) and 1 <= len(node[3]) < len(node[2])
        assert len(at) - len(node[1]) >= 3


@pytest.mark.parametrize('shape,kind,p,levels,m,exceptions', CASES, ids=IDS)
def test_files(kom, tmp_path, monkeypatch, shape, kind, p, levels, m, exceptions):
    from kompressor_amd import container
    monkeypatch.setattr(container, '_ROW_CROP_PLANE', 1)  # rows are cropped at every level
    ndim = len(shape) - 2
    x = field(shape, exceptions, seed=len(shape) + p)
    rel, eps = REL[m], 2.0 ** -(m + 1)
    assert P.mantissa_bits(rel) == m
    n_want, exc_want = P.quantise(x, m)
    want = P.restore(n_want, m, exc_want)
    E = 0 if exc_want is None else exc_want[0].size
    assert n_want.dtype == (np.int16 if m == 6 else np.int32) and E == (len(RAW) if exceptions else 0)
    pred = predictor(kom, kind, p, ndim, n_want)
    path = str(tmp_path / 'p.kmp')
    res = container.compress(path, x, pred, levels=levels, tile_crc=True, rel_error=rel)
    ok = np.ones(x.size, bool)
    if E:
        ok[exc_want[0]] = False
    worst = float(P.rel_errors(x.reshape(-1)[ok], want.reshape(-1)[ok]).max(initial=0.0))
    assert worst <= eps
    assert res['rel_error'] == eps and res['rel_error_asked'] == rel and res['exceptions'] == E
    assert isinstance(res['max_rel_error'], float) and res['max_rel_error'] == worst and res['max_rel_error'] <= res['rel_error']
    assert res['quant_dtype'] == n_want.dtype.name and res['levels'] == levels and res['bytes'] == os.path.getsize(path)
    assert 'abs_error' not in res and 'max_abs_error' not in res
    assert version_of(path) == 6
    info = container.info(path)
    assert info['version'] == 6 and info['shape'] == shape and info['sample_dtype'] == 'float32'
    assert info['rel_error'] == eps and info['quant_dtype'] == n_want.dtype.name and info['exceptions'] == E
    assert info['levels'] == levels and 'tile_crc' in info and 'max_error' not in info and 'abs_error' not in info
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
        names, sel = picks(shape, ndim, sp)
        for kw in sel:
            got = container.read_region(path, level=level, **kw)
            assert container.last_timing['partial'] is True and container.last_timing['tile_crc'] is True
            b0, b1 = kw.get('batch', (0, shape[0]))
            box = [kw.get(nm, (0, s)) for nm, s in zip(names, sp)]
            cut = top[(slice(b0, b1), *[slice(a, b) for a, b in box])]
            assert got.dtype == np.float32 and got.shape == cut.shape and np.array_equal(u32(got), u32(cut)), (level, kw)
            raw = np.isin(u32(cut), RAW)
            saw_exception |= bool(raw.any())
            saw_none |= not raw.any()
    if exceptions:
        assert saw_exception and saw_none  # boxes that contain exceptions, and boxes that miss them all


@pytest.mark.parametrize('exceptions', [False, True], ids=['clean', 'exc'])
def test_without_tile_crc_and_device_input(kom, tmp_path, exceptions):
    import torch
    from kompressor_amd import container
    x = field(VOL, exceptions, seed=5)
    n, exc = P.quantise(x, 6)
    want = P.restore(n, 6, exc)
    path = str(tmp_path / 'd.kmp')
    res = container.compress(path, torch.from_numpy(x).cuda(), kom.MeanPredictor(0, 3), rel_error=1e-2)
    assert res['rel_error'] == P.effective_rel(1e-2) == 2.0 ** -7 and 'tile_crc' not in container.info(path)
    got = container.decompress(path, as_numpy=False)
    assert got.is_cuda and got.dtype == torch.float32 and np.array_equal(u32(got.cpu().numpy()), u32(want))
    assert np.array_equal(u32(container.read_region(path, planes=(2, 5), cols=(3, 9))), u32(want[:, 2:5, :, 3:9]))
    assert container.last_timing['tile_crc'] is False
    assert container.check(path) == {'ok': True, 'crc32': True, 'tile_crc': None}
    planes = str(tmp_path / 'p.kmp')  # a bundle without tiles: read whole, then sliced
    container.compress(planes, x, kom.MeanPredictor(0, 3), levels=2, method='planes', rel_error=1e-2)
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
    x = field(VOL, True, seed=9)
    path = str(tmp_path / 'c.kmp')
    container.compress(path, x, kom.MeanPredictor(0, 3), levels=2, tile_crc=True, rel_error=1e-2)
    raw = open(path, 'rb').read()
    mlen = struct.unpack('<4sHHQ', raw[:16])[3]
    base = 16 + mlen
    count = packing._RHEAD.unpack(raw[base:base + packing._RHEAD.size])[2]
    plan = packing._rice_dec_plan(None, raw[base:base + packing._RHEAD.size + packing._RREC.size * count])
    assert count == 1 + 7 * 2 + 3 and plan['shapes'][-1] == plan['shapes'][-2] == plan['shapes'][-3] == (len(RAW),)
    assert container.info(path)['exceptions'] == len(RAW)
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
def test_all_bounds_none_writes_todays_bytes(kom, tmp_path, dtype):
    import near_spec as NS
    from kompressor_amd import container
    x = field(VOL, True, seed=3) if dtype == np.float32 else NS.noisy_field(VOL, np.uint16, seed=3)
    pred = kom.MeanPredictor(0, 3)
    a, b = str(tmp_path / 'a.kmp'), str(tmp_path / 'b.kmp')
    ra = container.compress(a, x, pred, levels=2, tile_crc=True)
    rb = container.compress(b, x, pred, levels=2, tile_crc=True, max_error=0, abs_error=None, rel_error=None)
    assert open(a, 'rb').read() == open(b, 'rb').read() and version_of(b) == 3 and ra == rb
    assert not {'rel_error', 'abs_error', 'quant_dtype', 'exceptions'} & set(container.info(b))
    assert np.array_equal(container.decompress(b).view(np.uint32 if dtype == np.float32 else dtype),
                          x.view(np.uint32 if dtype == np.float32 else dtype))  # lossless float32: bit for bit


def test_a_broken_bound_writes_nothing(kom, tmp_path, monkeypatch):
    from kompressor_amd import container
    x = field(VOL, False, seed=1)
    monkeypatch.setattr(container, '_prec_max_error', lambda *a: 1.0)
    with pytest.raises(RuntimeError):
        container.compress(str(tmp_path / 'x.kmp'), x, kom.MeanPredictor(0, 3), rel_error=1e-2)
    assert not os.listdir(tmp_path)


def test_file_size_on_the_decades_field(kom, tmp_path):
    from kompressor_amd import container
    x = P.decades_field()
    pred = kom.MeanPredictor(0, 3)
    bits = {r: container.compress(str(tmp_path / 'f.kmp'), x, pred, levels=2, rel_error=r)['bits_per_sample']
            for r in (None, 2.0 ** -4, 2.0 ** -6, 2.0 ** -8)}
    print('bits per sample:', {str(r): round(v, 3) for r, v in bits.items()})
    assert bits[2.0 ** -4] < bits[2.0 ** -6] < bits[2.0 ** -8] < 16.0 < bits[None]
