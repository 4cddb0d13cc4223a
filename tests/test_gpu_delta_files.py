"""Time-series files: ``compress(..., temporal='delta')`` / decompress / read_region / info / check
against the same call without ``temporal`` and tests/delta_spec.py -- lossless files bit-identical, float32 files
restored to the bits of the independent file, the version-8 header, partial reads along the chain, the
per-tile CRCs, malformed headers, the targets and the size on the spec's sequence."""

import filecmp
import json
import os
import struct

import numpy as np
import pytest

import delta_spec as D

pytestmark = pytest.mark.gpu

VOLUME, IMAGE = (5, 9, 10, 13, 1), (4, 21, 18, 1)
LEVELS = 2
KS = (None, 2, 5)
K_IDS = ['K-none', 'K-2', 'K-5']
BOUNDS = {'abs': {'abs_error': 2.0 ** -7}, 'rel': {'rel_error': 1e-3},
          'abs-runs': {'abs_error': 2.0 ** -7, 'exceptions': 'runs'}, 'rel-runs': {'rel_error': 1e-3, 'exceptions': 'runs'}}
BASE_VERSION = {'abs': 5, 'rel': 6, 'abs-runs': 7, 'rel-runs': 7}


def version_of(path):
    with open(path, 'rb') as f:
        return struct.unpack('<4sHHQ', f.read(16))[1]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def ndim_of(shape):
    return len(shape) - 2


def predictor(kom, shape):
    return kom.MeanPredictor(0, ndim_of(shape))


def field(shape, runs=False):
    """The spec's sequence (shift 0.05, no noise) cut to ``shape``; ``runs``: a NaN patch that stays, a NaN
    patch that moves with the frame, an infinity and a value no step here can quantise."""
    sp = shape[1:-1]
    x = D.sequence(0.05, 0.0, frames=shape[0], shape=sp if len(sp) == 3 else (1, *sp)).reshape(shape).copy()
    if runs:
        for t in range(shape[0]):
            v = x[t, ..., 0]
            v[..., 2:5, 3:9] = np.nan
            v[..., 6 + t % 2, t:t + 4] = np.nan
        f = x.reshape(-1)
        f[[0, f.size // 2, f.size - 1]] = [np.inf, 3e38, -np.inf]
    return x


def integers(shape, dtype, seed=0):
    """A slowly changing sequence of the whole range of ``dtype``: the frames differ by small steps that wrap."""
    rng = np.random.default_rng(seed)
    info = np.iinfo(dtype)
    W = 8 * np.dtype(dtype).itemsize
    base = rng.integers(info.min, int(info.max) + 1, size=shape[1:], dtype=np.int64)
    steps = np.cumsum(rng.integers(-3, 4, size=shape, dtype=np.int64), axis=0)
    x = (base[None] + steps - info.min) % (1 << W) + info.min
    x.reshape(-1)[:3] = info.min, info.max, 0
    return x.astype(dtype)


def pairs(T):
    return [(a, b) for a in range(T) for b in range(a + 1, T + 1)]


# ---- lossless ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize('K', KS, ids=K_IDS)
@pytest.mark.parametrize('shape', (VOLUME, IMAGE), ids=('volume', 'image'))
@pytest.mark.parametrize('dtype', (np.uint8, np.uint16, np.int16), ids=('uint8', 'uint16', 'int16'))
def test_lossless(kom, tmp_path, dtype, shape, K):
    c, pred = kom.container, predictor(kom, shape)
    x = integers(shape, dtype, seed=len(shape))
    a, b = str(tmp_path / 'delta.kmp'), str(tmp_path / 'plain.kmp')
    ra = c.compress(a, x, pred, levels=LEVELS, tile_crc=True, temporal='delta', key_interval=K)
    rb = c.compress(b, x, pred, levels=LEVELS, tile_crc=True)
    assert version_of(a) == 8 and version_of(b) == 3
    back = c.decompress(a)
    assert back.dtype == np.dtype(dtype) and back.shape == shape and np.array_equal(back, x)
    assert ra['temporal'] == 'delta' and ra['key_interval'] == K and 'temporal' not in rb
    assert ra['bytes'] == os.path.getsize(a) and ra['psnr'] == float('inf')
    info = c.info(a)
    assert info['version'] == 8 and info['temporal'] == 'delta' and info['key_interval'] == K
    assert info['sample_dtype'] == np.dtype(dtype).name and info['shape'] == shape and info['levels'] == LEVELS
    assert 'temporal' not in c.info(b) and 'key_interval' not in c.info(b)
    assert c.level_shapes(a) == c.level_shapes(b)
    # the bundle holds the pyramid of the spec's deltas, in the signed dtype of the samples' width
    lowres, (maps, _), meta = c.load(a)
    want = D.encode(x, K)
    assert meta['temporal'] == {'mode': 'delta', 'key_interval': K or 0, 'dtype': want.dtype.name}
    assert lowres.cpu().numpy().dtype == want.dtype
    assert np.array_equal(lowres.cpu().numpy(), D.level(want, ndim_of(shape), LEVELS))
    got = c.check(a)
    assert got['ok'] and got['crc32'] and got['tile_crc']['bad'] == []
    size = c.compressed_size(x, pred, levels=LEVELS, tile_crc=True, temporal='delta', key_interval=K)
    assert size['bundle_bytes'] == info['bundle_bytes'] and 0 <= size['bound_bytes'] - os.path.getsize(a) <= 16
    assert size['temporal'] == 'delta' and size['key_interval'] == K
    assert ra['bytes'] < rb['bytes']  # whole-range samples that change by small steps


def test_int32_lossless(kom, tmp_path):
    c, pred = kom.container, predictor(kom, VOLUME)
    x = integers(VOLUME, np.int32, seed=5)
    path = str(tmp_path / 'i32.kmp')
    c.compress(path, x, pred, levels=LEVELS, temporal='delta', key_interval=2)
    assert version_of(path) == 8 and np.array_equal(c.decompress(path), x)
    assert np.array_equal(c.read_region(path, batch=(3, 5), rows=(2, 7)), x[3:5, :, 2:7])


# ---- float32 ----------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def float_files(kom, tmp_path_factory):
    """Per (shape, mode): the field, the independent file's restored array, and per K the delta file."""
    root = tmp_path_factory.mktemp('delta')
    out = {}
    for sname, shape in (('volume', VOLUME), ('image', IMAGE)):
        for mode, kw in BOUNDS.items():
            x, pred = field(shape, runs='runs' in mode), predictor(kom, shape)
            plain = str(root / f'{sname}-{mode}-plain.kmp')
            rp = kom.container.compress(plain, x, pred, levels=LEVELS, tile_crc=True, **kw)
            entry = {'x': x, 'plain': plain, 'rp': rp, 'want': kom.container.decompress(plain), 'kw': kw, 'K': {}}
            for K in KS:
                path = str(root / f'{sname}-{mode}-{K}.kmp')
                res = kom.container.compress(path, x, pred, levels=LEVELS, tile_crc=True, temporal='delta',
                                             key_interval=K, **kw)
                entry['K'][K] = (path, res)
            out[sname, mode] = entry
    return out


@pytest.mark.parametrize('K', KS, ids=K_IDS)
@pytest.mark.parametrize('mode', list(BOUNDS))
@pytest.mark.parametrize('sname', ('volume', 'image'))
def test_float32_restores_the_independent_files_bits(kom, float_files, sname, mode, K):
    c, F = kom.container, float_files[sname, mode]
    path, res = F['K'][K]
    x, want, rp = F['x'], F['want'], F['rp']
    got = c.decompress(path)
    assert got.dtype == np.float32 and got.shape == x.shape and np.array_equal(bits(got), bits(want))
    assert version_of(path) == 8 and version_of(F['plain']) == BASE_VERSION[mode]
    if 'runs' in mode:
        assert rp['exceptions'] > rp['exception_runs'] >= 1 and not np.isfinite(got).all()
    # the int16 / int32 choice, the exceptions, the bound's check and the quality record: those of the plain call
    for k, v in rp.items():
        if k not in ('bytes', 'ratio', 'bits_per_sample'):
            assert res[k] == v or (v != v and res[k] != res[k]), k
    assert res['temporal'] == 'delta' and res['key_interval'] == K and res['bytes'] == os.path.getsize(path)
    info, pinfo = c.info(path), c.info(F['plain'])
    assert info['temporal'] == 'delta' and info['key_interval'] == K and info['version'] == 8
    for k in ('shape', 'sample_dtype', 'levels', 'quant_dtype', 'exceptions', 'exception_runs', 'abs_error', 'rel_error'):
        assert info.get(k) == pinfo.get(k), k
    meta = c.load(path)[2]
    assert meta['temporal'] == {'mode': 'delta', 'key_interval': K or 0, 'dtype': info['quant_dtype']}
    chk = c.check(path)
    assert chk['ok'] and chk['tile_crc']['bad'] == []
    size = c.compressed_size(x, predictor(kom, x.shape), levels=LEVELS, tile_crc=True, temporal='delta', key_interval=K,
                             **F['kw'])
    assert size['bundle_bytes'] == info['bundle_bytes'] and 0 <= size['bound_bytes'] - os.path.getsize(path) <= 16


# ---- partial reads ----------------------------------------------------------------------------------------

def region_cases(shape):
    """Per level: the selections of a rows / cols box in that level's coordinates."""
    if len(shape) == 5:
        return {0: [{}, {'planes': (2, 7), 'rows': (1, 6), 'cols': (3, 11)}], 1: [{'rows': (1, 4), 'cols': (0, 5)}]}
    return {0: [{}, {'rows': (3, 17), 'cols': (2, 9)}], 1: [{'rows': (2, 9), 'cols': (1, 8)}]}


def check_regions(c, path, full, K):
    names = ('planes', 'rows', 'cols')[5 - full.ndim:]
    nsp = len(names)
    for level, boxes in region_cases(full.shape).items():
        top = full[(slice(None), *[slice(None, None, 2 ** level)] * nsp)]
        for kw in boxes:
            box = tuple(slice(*kw.get(nm, (0, s))) for nm, s in zip(names, top.shape[1:1 + nsp]))
            for a, b in pairs(full.shape[0]):
                got = c.read_region(path, batch=(a, b), level=level, **kw)
                assert c.last_timing['partial'] is True and c.last_timing['tile_crc'] is True
                cut = top[(slice(a, b), *box)]
                assert got.dtype == full.dtype and got.shape == cut.shape, (level, kw, a, b)
                assert np.array_equal(bits(got), bits(cut)), (level, kw, a, b, K)
    # the stored coarsest lowres: no codec kernel, the chain alone
    top = full[(slice(None), *[slice(None, None, 2 ** LEVELS)] * nsp)]
    assert np.array_equal(bits(c.read_region(path, batch=(1, 3), level=LEVELS)), bits(top[1:3]))


@pytest.mark.parametrize('crop_rows', (False, True), ids=('planes', 'row-runs'))
@pytest.mark.parametrize('K', KS, ids=K_IDS)
@pytest.mark.parametrize('shape', (VOLUME, IMAGE), ids=('volume', 'image'))
def test_read_region_lossless(kom, tmp_path, monkeypatch, shape, K, crop_rows):
    c = kom.container
    if crop_rows:
        monkeypatch.setattr(c, '_ROW_CROP_PLANE', 1)  # rows are cropped at every level
    x = integers(shape, np.uint16, seed=3)
    path = str(tmp_path / 'x.kmp')
    c.compress(path, x, predictor(kom, shape), levels=LEVELS, tile_crc=True, temporal='delta', key_interval=K)
    check_regions(c, path, x, K)


@pytest.mark.parametrize('K', KS, ids=K_IDS)
@pytest.mark.parametrize('mode', ('abs-runs', 'rel'))
@pytest.mark.parametrize('sname', ('volume', 'image'))
def test_read_region_float32(kom, float_files, monkeypatch, sname, mode, K):
    c, F = kom.container, float_files[sname, mode]
    monkeypatch.setattr(c, '_ROW_CROP_PLANE', 1)
    check_regions(c, F['K'][K][0], F['want'], K)


def test_a_plan_starts_at_the_key_frame(kom, tmp_path):
    c = kom.container
    x = integers(VOLUME, np.int16, seed=8)
    plain, paths = str(tmp_path / 'plain.kmp'), {}
    c.compress(plain, x, predictor(kom, VOLUME), levels=LEVELS)
    for K in KS:
        paths[K] = str(tmp_path / f'{K}.kmp')
        c.compress(paths[K], x, predictor(kom, VOLUME), levels=LEVELS, temporal='delta', key_interval=K)
    meta = {K: c.load(p)[2] for K, p in paths.items()}
    plan = c.plan_region(meta[2], batch=(3, 4))
    assert plan['batch'] == (2, 4) and plan['frames'] == (3, 4)
    for ar in plan['arrays']:  # no tile, no sample of frames 0 - 1
        per = int(np.prod(ar['shape'][1:]))
        assert ar['ranges'] and all(first >= 2 * per and end <= 4 * per for first, end, _ in ar['ranges'])
    for (a, b), K in (((3, 4), None), ((3, 4), 5), ((4, 5), 2), ((0, 1), 2), ((1, 5), 2), ((2, 3), 2)):
        plan = c.plan_region(meta[K], batch=(a, b), rows=(1, 5))
        assert plan['batch'] == D.frames_read(a, b, K) and plan['frames'] == (a, b)
        assert plan['arrays'][0]['local_shape'][0] == b - D.frames_read(a, b, K)[0]
    # a file without temporal: the plan of the frames asked for, and no 'frames' entry
    pmeta = c.load(plain)[2]
    plan = c.plan_region(pmeta, batch=(3, 4))
    assert plan['batch'] == (3, 4) and 'frames' not in plan
    want = c.plan_region({k: v for k, v in meta[2].items() if k != 'temporal'}, batch=(2, 4))
    got = c.plan_region(meta[2], batch=(2, 4))
    assert {k: v for k, v in got.items() if k != 'frames'} == want


# ---- the other forms stay what they were ------------------------------------------------------------------

def test_without_temporal_and_single_frames_are_the_ordinary_files(kom, tmp_path):
    c = kom.container
    a, b = str(tmp_path / 'a.kmp'), str(tmp_path / 'b.kmp')
    cases = [(integers(VOLUME, np.uint16), {}, 3), (integers(IMAGE, np.int16), {}, 3),
             (field(VOLUME), BOUNDS['abs'], 5), (field(VOLUME), BOUNDS['rel'], 6),
             (field(VOLUME, runs=True), BOUNDS['abs-runs'], 7), (field(IMAGE, runs=True), BOUNDS['rel-runs'], 7)]
    for x, kw, version in cases:
        pred = predictor(kom, x.shape)
        ra = c.compress(a, x, pred, levels=LEVELS, tile_crc=True, **kw)
        rb = c.compress(b, x, pred, levels=LEVELS, tile_crc=True, temporal=None, key_interval=None, **kw)
        assert filecmp.cmp(a, b, shallow=False) and version_of(b) == version and ra == rb
        assert 'temporal' not in c.load(b)[2]
        # one frame: nothing to take a delta along
        one = np.ascontiguousarray(x[:1])
        c.compress(a, one, pred, levels=LEVELS, tile_crc=True, **kw)
        for K in (None, 1, 3):
            r1 = c.compress(b, one, pred, levels=LEVELS, tile_crc=True, temporal='delta', key_interval=K, **kw)
            assert filecmp.cmp(a, b, shallow=False) and version_of(b) == version and 'temporal' not in r1
            assert c.compressed_size(one, pred, levels=LEVELS, tile_crc=True, temporal='delta', key_interval=K,
                                     **kw)['bundle_bytes'] == c.info(a)['bundle_bytes']
        assert np.array_equal(bits(c.decompress(b)), bits(c.decompress(a)))


def test_key_interval_one_is_every_frame_on_its_own(kom, tmp_path):
    """``K = 1``: every frame is a key frame -- a version-8 file of the samples' own bits."""
    c = kom.container
    x = integers(IMAGE, np.uint16, seed=2)
    path = str(tmp_path / 'k1.kmp')
    c.compress(path, x, predictor(kom, IMAGE), levels=LEVELS, temporal='delta', key_interval=1)
    assert version_of(path) == 8 and np.array_equal(c.decompress(path), x)
    assert np.array_equal(c.read_region(path, batch=(2, 3)), x[2:3])
    assert c.plan_region(c.load(path)[2], batch=(2, 3))['batch'] == (2, 3)


def rewrite(src, dst, version=None, **over):
    """``src`` with entries of its metadata replaced (``...`` removes one) and, optionally, another version."""
    raw = open(src, 'rb').read()
    magic, v, zero, mlen = struct.unpack('<4sHHQ', raw[:16])
    meta = json.loads(raw[16:16 + mlen])
    meta.update(over)
    meta = {k: val for k, val in meta.items() if val is not ...}
    js = json.dumps(meta, separators=(',', ':')).encode()
    js += b' ' * (-len(js) % 8)
    with open(dst, 'wb') as f:
        f.write(struct.pack('<4sHHQ', magic, v if version is None else version, zero, len(js)) + js + raw[16 + mlen:])
    return dst


def test_malformed_headers_are_refused(kom, float_files, tmp_path):
    c = kom.container
    src = float_files['volume', 'abs']['K'][2][0]
    good = c.load(src)[2]['temporal']
    dst = str(tmp_path / 'bad.kmp')
    assert np.array_equal(bits(c.decompress(rewrite(src, dst))), bits(float_files['volume', 'abs']['want']))
    bad = [..., None, 'delta', [], {}, dict(good, mode='xor'), dict(good, mode=None), dict(good, key_interval=-1),
           dict(good, key_interval=True), dict(good, key_interval=2.0), dict(good, key_interval='2'),
           dict(good, key_interval=None), dict(good, dtype='uint16'), dict(good, dtype='float32'), dict(good, dtype=None),
           dict(good, dtype='int32'),  # the quantiser's integers here are int16
           {k: v for k, v in good.items() if k != 'key_interval'}, {k: v for k, v in good.items() if k != 'dtype'}]
    for t in bad:
        for call in (c.info, c.decompress, c.check, c.level_shapes, lambda p: c.read_region(p, batch=(0, 1))):
            with pytest.raises(ValueError, match='temporal|deltas'):
                call(rewrite(src, dst, temporal=t))
    for over in ({'max_error': 0}, {'max_error': 2}, {'max_error': None}):
        with pytest.raises(ValueError, match='max_error'):
            c.decompress(rewrite(src, dst, **over))
    # a temporal entry in any other version; version 8 refused by what is wrong with it, not as unknown
    for version in (2, 3, 5):
        with pytest.raises(ValueError, match='temporal'):
            c.decompress(rewrite(src, dst, version=version, **({'quant': ...} if version != 5 else {})))
    with pytest.raises(ValueError, match='temporal'):
        c.info(rewrite(float_files['volume', 'abs']['plain'], dst, version=8))
    # a lossless version-8 file whose deltas are not the signed dtype of its samples' width
    x = integers(IMAGE, np.uint16)
    lossless = str(tmp_path / 'u16.kmp')
    c.compress(lossless, x, predictor(kom, IMAGE), levels=LEVELS, temporal='delta')
    for t in (dict(good, dtype='int8'), dict(good, dtype='int32'), dict(good, dtype='uint16')):
        with pytest.raises(ValueError, match='temporal|deltas'):
            c.decompress(rewrite(lossless, dst, temporal=t))
    with pytest.raises(ValueError, match='temporal|deltas'):
        c.decompress(rewrite(lossless, dst, sample_dtype='float32'))
    # the interval is the file's: another one decodes to another array, not to an error
    other = c.decompress(rewrite(lossless, dst, temporal=dict(c.load(lossless)[2]['temporal'], key_interval=2)))
    assert other.shape == x.shape and np.array_equal(other[:2], x[:2]) and not np.array_equal(other, x)


def test_argument_errors_write_nothing(kom, tmp_path):
    c, path = kom.container, str(tmp_path / 'x.kmp')
    u16, f32 = integers(IMAGE, np.uint16), field(IMAGE)
    pred = predictor(kom, IMAGE)
    for x, kw in ((u16, {'key_interval': 2}), (u16, {'temporal': 'Delta'}), (u16, {'temporal': 'xor'}),
                  (u16, {'temporal': True}), (u16, {'temporal': 1}), (u16, {'temporal': b'delta'}),
                  (u16, {'temporal': 'delta', 'key_interval': 0}), (u16, {'temporal': 'delta', 'key_interval': True}),
                  (u16, {'temporal': 'delta', 'key_interval': 2.0}), (u16, {'temporal': 'delta', 'key_interval': '2'}),
                  (u16, {'temporal': 'delta', 'max_error': 2}), (u16, {'temporal': 'delta', 'target_bits': 4.0}),
                  (u16, {'temporal': 'delta', 'target_psnr': 40.0}),
                  (f32, {'temporal': 'delta'}), (f32.view(np.uint32), {'temporal': 'delta'}),
                  (f32, {'key_interval': 2, 'abs_error': 1e-3})):
        with pytest.raises(ValueError):
            c.compress(path, x, pred, levels=LEVELS, **kw)
        if not any(k.startswith('target') for k in kw):
            with pytest.raises(ValueError):
                c.compressed_size(x, pred, levels=LEVELS, **kw)
    assert not os.listdir(tmp_path)


# ---- targets, and the size ----------------------------------------------------------------------------------

@pytest.mark.parametrize('target', [{'target_bits': 10.0}, {'target_ratio': 1.5, 'target_mode': 'rel'},
                                    {'target_psnr': 50.0}], ids=['bits-abs', 'ratio-rel', 'psnr-abs'])
def test_targets_write_the_explicit_bounds_file(kom, tmp_path, target):
    c, x, pred = kom.container, field(VOLUME, runs=True), predictor(kom, VOLUME)
    a, b = str(tmp_path / 'target.kmp'), str(tmp_path / 'bound.kmp')
    rt =c.compress(a, x, pred, levels=LEVELS, exceptions='runs', temporal='delta', key_interval=2, **target)
    key = 'rel_error' if target.get('target_mode') == 'rel' else 'abs_error'
    rb = c.compress(b, x, pred, levels=LEVELS, exceptions='runs', temporal='delta', key_interval=2, **{key: rt[key]})
    assert filecmp.cmp(a, b, shallow=False) and version_of(a) == 8
    assert rt['temporal'] == 'delta' and rt['key_interval'] == 2 and rt['bytes'] == rb['bytes']
    if 'target_psnr' not in target:
        assert rt['bytes'] <= rt['target_bytes']
        # the candidates were sized as time series: the chosen rung's size is this file's
        assert 0 <= rt['bound_bytes'] - rt['bytes'] <= 16
    assert np.array_equal(bits(c.decompress(a)), bits(c.decompress(b)))


def test_size_on_the_spec_sequence(kom, tmp_path):
    """Shift 0.05, no noise, ``abs_error = 2^-7``: the delta file is smaller than the independent one."""
    c, x, pred = kom.container, D.sequence(0.05, 0.0), kom.MeanPredictor(0, 3)
    a, b = str(tmp_path / 'delta.kmp'), str(tmp_path / 'plain.kmp')
    ra = c.compress(a, x, pred, levels=2, abs_error=2.0 ** -7, temporal='delta')
    rb = c.compress(b, x, pred, levels=2, abs_error=2.0 ** -7)
    print(f'spec sequence, abs_error 2^-7: independent {rb["bits_per_sample"]:.3f}, delta {ra["bits_per_sample"]:.3f} '
          f'bits per sample ({rb["bytes"]} -> {ra["bytes"]} bytes)')
    assert ra['bytes'] < rb['bytes'] and ra['quant_dtype'] == rb['quant_dtype'] == 'int16'
    assert np.array_equal(bits(c.decompress(a)), bits(c.decompress(b)))
    # the bundle holds the pyramid of the spec's deltas of the spec's integers
    import quant_spec as Q
    n, exc = Q.quantise(x, Q.exponent(2.0 ** -7))
    assert exc is None
    assert np.array_equal(c.load(a)[0].cpu().numpy(), D.level(D.encode(n), 3, 2))
