"""Masked float32 files: ``compress(..., exceptions='runs')`` / decompress / read_region / info /
check against the ``'list'`` file of the same call and tests/runs_spec.py -- the restored arrays equal bit for
bit, the version-7 header, the sizes, partial reads that cut runs, a corrupted run array, and the targets."""

import filecmp
import os
import struct
import time

import numpy as np
import pytest
import torch

import prec_spec as P
import quant_spec as Q
import runs_spec as R

pytestmark = pytest.mark.gpu

SHAPE = (1, 20, 24, 28, 1)
LEVELS = 2
BOUNDS = {'abs': {'abs_error': 2.0 ** -7}, 'rel': {'rel_error': 1e-3}}


def version_of(path):
    with open(path, 'rb') as f:
        return struct.unpack('<4sHHQ', f.read(16))[1]


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def masked_field():
    """The first octant of the spec field with a NaN slab, an ellipsoid of NaNs, scattered +inf and NaNs of
    two payloads, and values past the int32 range of any step used here."""
    x = Q.spec_field()[:, :20, :24, :28].copy()
    assert x.shape == SHAPE
    v = x[0, ..., 0]
    z, y, xx = np.meshgrid(*[np.arange(s) for s in SHAPE[1:4]], indexing='ij')
    v[((z - 13) ** 2 / 25 + (y - 12) ** 2 / 60 + (xx - 14) ** 2 / 60) < 0.62] = np.nan
    v[4:6] = np.nan  # planes 4 and 5: one run
    f, rng = x.reshape(-1), np.random.default_rng(3)
    at = rng.choice(f.size, 60, replace=False)
    f[at[:20]] = np.inf
    u32(f)[at[20:40]] = 0x7fc00001
    u32(f)[at[40:50]] = 0xffc12345
    f[at[50:]] = 3e38
    f[[0, 1, f.size - 2, f.size - 1]] = [np.inf, np.inf, -np.inf, -np.inf]  # runs at both ends of the array
    return x


def spec_of(mode, x):
    """``(restored array, exceptions)`` of the numpy rule."""
    if mode == 'abs':
        e = Q.exponent(BOUNDS['abs']['abs_error'])
        n, exc = Q.quantise(x, e)
        return Q.restore(n, e, exc), exc
    m = P.mantissa_bits(BOUNDS['rel']['rel_error'])
    n, exc = P.quantise(x, m)
    return P.restore(n, m, exc), exc


@pytest.fixture(scope='module')
def files(kom, tmp_path_factory):
    """Per mode: the field, the spec's restored array and exceptions, the 'list' and the 'runs' file."""
    root = tmp_path_factory.mktemp('runs')
    x, pred, out = masked_field(), kom.MeanPredictor(0, 3), {}
    for mode, kw in BOUNDS.items():
        paths = {k: str(root / f'{mode}-{k}.kmp') for k in ('list', 'runs')}
        res = {k: kom.container.compress(paths[k], x, pred, levels=LEVELS, tile_crc=True, exceptions=k, **kw)
               for k in paths}
        want, exc = spec_of(mode, x)
        out[mode] = {'x': x, 'want': want, 'exc': exc, 'paths': paths, 'res': res, 'kw': kw}
    return out


@pytest.mark.parametrize('mode', list(BOUNDS))
def test_runs_file_against_the_list_file(kom, files, mode):
    c, F = kom.container, files[mode]
    x, want, (idx, bits) = F['x'], F['want'], F['exc']
    full = {k: c.decompress(F['paths'][k]) for k in ('list', 'runs')}
    assert full['runs'].dtype == np.float32 and full['runs'].shape == SHAPE
    assert np.array_equal(u32(full['runs']), u32(full['list'])) and np.array_equal(u32(full['runs']), u32(want))
    # every exception bit for bit, every other value within the bound
    assert np.array_equal(u32(full['runs']).reshape(-1)[idx], bits) and np.array_equal(u32(x).reshape(-1)[idx], bits)
    ok = np.ones(x.size, bool)
    ok[idx] = False
    xd, rd = x.reshape(-1)[ok].astype(np.float64), full['runs'].reshape(-1)[ok].astype(np.float64)
    if mode == 'abs':
        assert np.abs(rd - xd).max() <= Q.effective(F['kw']['abs_error'])
    else:
        assert (np.abs(rd - xd) <= P.effective_rel(F['kw']['rel_error']) * np.maximum(np.abs(xd), 2.0 ** -126)).all()
    # the header, the result, the sizes
    runs_want = R.runs((idx, bits))[0].size
    assert 1 <= runs_want < idx.size
    rl, rr = F['res']['list'], F['res']['runs']
    assert version_of(F['paths']['runs']) == 7 and version_of(F['paths']['list']) == {'abs': 5, 'rel': 6}[mode]
    info = c.info(F['paths']['runs'])
    assert info['version'] == 7 and info['exception_runs'] == runs_want and info['exceptions'] == idx.size
    assert info['shape'] == SHAPE and info['sample_dtype'] == 'float32' and info['levels'] == LEVELS and 'tile_crc' in info
    assert 'exception_runs' not in c.info(F['paths']['list']) and 'exception_runs' not in rl
    assert rr['exception_runs'] == runs_want and rr['exceptions'] == rl['exceptions'] == idx.size
    assert rr['quant_dtype'] == rl['quant_dtype']  # the fill leaves the integer extent alone
    for k in ('max_abs_error', 'max_rel_error', 'mse', 'psnr', 'value_range', 'abs_error', 'rel_error'):
        assert rr.get(k) == rl.get(k), k  # measured on what decompress returns: the same array
    assert rr['bytes'] == os.path.getsize(F['paths']['runs']) < os.path.getsize(F['paths']['list']) == rl['bytes']
    assert c.level_shapes(F['paths']['runs']) == c.level_shapes(F['paths']['list'])
    # compressed_size: the file's bytes (the CRC's decimal digits aside, as for every file)
    pred = kom.MeanPredictor(0, 3)
    for k in ('list', 'runs'):
        size = c.compressed_size(x, pred, levels=LEVELS, tile_crc=True, exceptions=k, **F['kw'])
        file_bytes = os.path.getsize(F['paths'][k])
        assert size['bundle_bytes'] == c.info(F['paths'][k])['bundle_bytes']
        assert 0 <= size['bound_bytes'] - file_bytes <= 16
        assert size.get('exception_runs') == (runs_want if k == 'runs' else None)
    # check, and load's arrays: the four run arrays last
    got = c.check(F['paths']['runs'])
    assert got['ok'] and got['crc32'] and got['tile_crc']['bad'] == []
    _, (maps, _), meta = c.load(F['paths']['runs'])
    assert len(maps) == 7 * LEVELS + 4 and meta['exception_runs'] == runs_want
    for a, b in zip(maps[-4:], R.runs((idx, bits))):
        assert np.array_equal(a.cpu().numpy(), b)


@pytest.mark.parametrize('mode', list(BOUNDS))
def test_read_region(kom, files, mode, monkeypatch):
    c, F = kom.container, files[mode]
    monkeypatch.setattr(c, '_ROW_CROP_PLANE', 1)  # rows are cropped at every level
    want = F['want']
    boxes = [
        {'planes': (5, 6), 'rows': (3, 20), 'cols': (2, 27)},   # inside the slab: its run cut at both ends
        {'planes': (4, 14)},                                    # the slab whole, the ellipsoid cut in z
        {'planes': (12, 14), 'rows': (10, 14), 'cols': (12, 17)},  # wholly inside the ellipsoid
        {'planes': (0, 1), 'rows': (0, 1)},                     # the run at index 0
        {'planes': (19, 20), 'cols': (20, 28)},                 # the run ending at numel
        {},
    ]
    saw_none = False
    for level in (0, 1, 2):
        top = want[:, ::2 ** level, ::2 ** level, ::2 ** level]
        for kw in boxes + [{'planes': (17, 19), 'rows': (0, 3), 'cols': (0, 3)}]:
            kw = {k: (lo >> level, max((hi - 1 >> level) + 1, (lo >> level) + 1)) for k, (lo, hi) in kw.items()}
            got = c.read_region(F['paths']['runs'], level=level, **kw)
            assert c.last_timing['partial'] is True and c.last_timing['tile_crc'] is True
            box = [kw.get(nm, (0, s)) for nm, s in zip(('planes', 'rows', 'cols'), top.shape[1:4])]
            cut = top[(slice(None), *[slice(a, b) for a, b in box])]
            assert got.shape == cut.shape and np.array_equal(u32(got), u32(cut)), (level, kw)
            lst = c.read_region(F['paths']['list'], level=level, **kw)
            assert np.array_equal(u32(got), u32(lst))
            saw_none |= bool(np.isfinite(cut).all())
    assert saw_none  # a box without any exception
    # level 1 shows exactly the exceptions on even coordinates
    idx, bits = F['exc']
    lidx, lbits, lshape = Q.level_exceptions((idx, bits), SHAPE, 3, 1)
    got = c.read_region(F['paths']['runs'], level=1)
    assert got.shape == lshape and np.array_equal(u32(got).reshape(-1)[lidx], lbits)
    assert np.array_equal(np.flatnonzero(~np.isfinite(got.reshape(-1))), lidx[~np.isfinite(lbits.view(np.float32))])


def test_a_corrupted_length_is_refused(kom, files, tmp_path):
    c = kom.container
    src = files['abs']['paths']['runs']
    lowres, (maps, _), meta = c.load(src)
    meta = {k: v for k, v in meta.items() if k not in ('bundle_bytes', 'crc32', 'tile_crc')}
    second_start = int(maps[-4].cpu().numpy()[:2].astype(np.int64).sum())  # both gaps' high words are 0 here
    assert not maps[-3].cpu().numpy()[:2].any()
    # (name, [(array, entry, value), ...]): lengths are maps[-2], start gap words maps[-4] (low) and maps[-3] (high)
    damage = (('long', [(-2, 0, 0xffffffff)]), ('empty', [(-2, 1, 0)]), ('far', [(-4, 0, 0xfffffff0)]),
              ('high', [(-3, 2, 1)]),
              # a start of 2**63 - 10: start + length wraps to a negative int64, which no upper bound catches
              ('wrap', [(-3, 0, 0x7fffffff), (-4, 0, 0xfffffff6), (-2, 0, 100)]),
              ('wrap later', [(-3, 2, 0x7fffffff), (-4, 2, 0xfffffff0)]),
              # a gap whose high word has its top bit set is negative: the run steps back onto its neighbour
              ('backwards', [(-3, 2, 0xffffffff), (-4, 2, 0xffffffff)]),
              # the first run one element longer than the gap to the second: in bounds, but not disjoint
              ('overlap', [(-2, 0, second_start + 1)]))
    for name, changes in damage:
        arrays = list(maps)
        for which, at, value in changes:
            a = arrays[which].cpu().numpy().copy()
            a[at] = value
            arrays[which] = torch.from_numpy(a).cuda()
        blob, total, crc, table = c._bundle(lowres, arrays, (), 'rice', True)
        path = str(tmp_path / f'{name}.kmp')
        c._write(path, meta, blob, total, crc, time.perf_counter(), table, 7)
        assert c.check(path)['ok']  # the CRCs are the damaged bundle's own: only the extents give it away
        with pytest.raises(ValueError):
            c.decompress(path)
        with pytest.raises(ValueError):
            c.read_region(path, planes=(3, 7))
    # the same rewrite with nothing changed decodes
    blob, total, crc, table = c._bundle(lowres, list(maps), (), 'rice', True)
    path = str(tmp_path / 'same.kmp')
    c._write(path, meta, blob, total, crc, time.perf_counter(), table, 7)
    assert filecmp.cmp(path, src, shallow=False)
    # a run array of another length than the metadata says
    blob, total, crc, table = c._bundle(lowres, [*maps[:-1], maps[-1][:-1].contiguous()], (), 'rice', False)
    c._write(path, meta, blob, total, crc, time.perf_counter(), table, 7)
    with pytest.raises(ValueError):
        c.decompress(path)


@pytest.mark.parametrize('mode', list(BOUNDS))
def test_without_exceptions_the_file_is_the_list_file(kom, tmp_path, mode):
    c = kom.container
    x = Q.spec_field()[:, :20, :24, :28].copy()
    a, b = str(tmp_path / 'list.kmp'), str(tmp_path / 'runs.kmp')
    pred = kom.MeanPredictor(0, 3)
    ra = c.compress(a, x, pred, levels=LEVELS, tile_crc=True, **BOUNDS[mode])
    rb = c.compress(b, x, pred, levels=LEVELS, tile_crc=True, exceptions='runs', **BOUNDS[mode])
    assert filecmp.cmp(a, b, shallow=False) and version_of(b) == {'abs': 5, 'rel': 6}[mode]
    assert rb['exceptions'] == 0 and rb['exception_runs'] == 0 and 'exception_runs' not in ra
    assert {k: v for k, v in rb.items() if k != 'exception_runs'} == ra
    sa = c.compressed_size(x, pred, levels=LEVELS, tile_crc=True, **BOUNDS[mode])
    sb = c.compressed_size(x, pred, levels=LEVELS, tile_crc=True, exceptions='runs', **BOUNDS[mode])
    assert sb['bound_bytes'] == sa['bound_bytes'] and sb['exception_runs'] == 0


@pytest.mark.parametrize('target', [{'target_bits': 6.0}, {'target_bits': 14.0, 'target_mode': 'rel'},
                                    {'target_psnr': 50.0}, {'target_psnr': 40.0, 'target_mode': 'rel'}],
                         ids=['bits-abs', 'bits-rel', 'psnr-abs', 'psnr-rel'])
def test_targets_write_the_explicit_bounds_file(kom, files, tmp_path, target):
    c, x, pred = kom.container, files['abs']['x'], kom.MeanPredictor(0, 3)
    a, b, l = str(tmp_path / 'target.kmp'), str(tmp_path / 'bound.kmp'), str(tmp_path / 'list.kmp')
    rt = c.compress(a, x, pred, levels=LEVELS, exceptions='runs', **target)
    key = 'rel_error' if target.get('target_mode') == 'rel' else 'abs_error'
    rb = c.compress(b, x, pred, levels=LEVELS, exceptions='runs', **{key: rt[key]})
    assert filecmp.cmp(a, b, shallow=False) and version_of(a) == 7
    assert rt['exception_runs'] == rb['exception_runs'] >= 1 and rt['bytes'] == rb['bytes']
    if 'target_bits' in target:
        assert rt['bytes'] <= rt['target_bytes']
    else:  # a quality target chooses its rung by the restored values alone: the list form's rung, a smaller file
        rl = c.compress(l, x, pred, levels=LEVELS, **target)
        assert version_of(l) in (5, 6) and 'exception_runs' not in rl
        assert rt[key] == rl[key] and rt['bytes'] < rl['bytes']
