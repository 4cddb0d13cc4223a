"""container.read_region with rows, cols and level: a box of any pyramid level of a compressed
file, bit-equal to the strided slice of ``decompress(path)``, reading only what the box needs.

The small volumes are ``[2, 21, 34, 40, 1]`` (odd, even and even extents; levels='auto' makes 4
levels whose extents change parity on the way down) with the row-crop threshold patched to 1, so
rows are cropped at every level although every plane is smaller than a tile; the ``264 x 264``
planes exceed one tile at level 0 and test the default threshold."""

import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TILE = 16384
RICE_LAUNCHES = {'rice_bundle_decode_ranges', 'rice_tile_crc'}


def _field(shape, dtype, seed=0):
    """A smooth field plus noise (small but non-zero residuals), any sample dtype, any rank."""
    rng = np.random.default_rng(seed)
    g = np.indices(shape[1:-1]).astype(np.float64)
    f = sum(a * np.sin(gi / w + i) for i, (gi, a, w) in enumerate(zip(g, (60, 40, 30), (5.0, 3.0, 4.0))))
    f = np.broadcast_to(f[None, ..., None], shape) + rng.normal(0, 1.5, shape)
    if dtype == np.float32:
        return f.astype(np.float32)
    info = np.iinfo(dtype)
    off = 0 if info.min < 0 else 200
    return ((np.rint(f + off).astype(np.int64) - info.min) % (info.max - info.min + 1) + info.min).astype(dtype)


def _linear(kom, p):
    n = (2 * p + 2) ** 3
    w = (np.full((n, 19), 1.0 / n) + np.random.default_rng(p).standard_normal((n, 19)) * 0.01).astype(np.float32)
    return kom.LinearPredictor(w, np.zeros(19, np.float32), p, 3, arith='f32')


@pytest.fixture
def crop_everywhere(kom, monkeypatch):
    monkeypatch.setattr(kom.container, '_ROW_CROP_PLANE', 1)


def _strided(full, k):
    return full[(slice(None), *[slice(None, None, 2 ** k)] * (full.ndim - 2))]


def _axis_options(n):
    """The first, the last, an interior span and the whole axis."""
    return [(0, 1), (n - 1, n), (n // 3, min(n // 3 + 3, n)), (0, n)]


def _boxes(shape):
    """The 64 boxes of an array: every combination of the options of its three axes."""
    opts = [_axis_options(n) for n in shape[1:4]]
    return [(a, b, c) for a in opts[0] for b in opts[1] for c in opts[2]]


CONFIGS = [(f'{np.dtype(dt).name}-mean-p{p}', dt, ('mean', p))
           for dt in (np.uint16, np.uint8, np.int16, np.float32) for p in (0, 1, 2)]
CONFIGS += [(f'uint16-linear-f32-p{p}', np.uint16, ('linear', p)) for p in (0, 1)]


@pytest.mark.parametrize('name,dtype,pred', CONFIGS, ids=[c[0] for c in CONFIGS])
def test_boxes_at_every_level(kom, tmp_path, crop_everywhere, name, dtype, pred):
    C = kom.container
    x = _field((2, 21, 34, 40, 1), dtype, seed=len(name))
    kind, p = pred
    path = str(tmp_path / 'v.kmp')
    made = C.compress(path, x, kom.MeanPredictor(p, 3) if kind == 'mean' else _linear(kom, p), levels='auto')
    full = C.decompress(path)
    assert np.array_equal(full.view(np.uint8), x.view(np.uint8))
    shapes = C.level_shapes(path)
    L = made['levels']
    assert L == 4 and len(shapes) == L + 1 and shapes[0] == x.shape
    assert shapes == [_strided(full, k).shape for k in range(L + 1)]
    for k in (0, 1, L):
        want_k = _strided(full, k)
        for i, (planes, rows, cols) in enumerate(_boxes(shapes[k])):
            batch = (None, (1, 2), (0, 1))[i % 3]
            got = C.read_region(path, planes=planes, rows=rows, cols=cols, batch=batch, level=k)
            tm = dict(C.last_timing)
            b = slice(*batch) if batch else slice(None)
            want = want_k[b, planes[0]:planes[1], rows[0]:rows[1], cols[0]:cols[1]]
            assert got.dtype == x.dtype and got.shape == want.shape and got.flags['C_CONTIGUOUS']
            assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), (name, k, planes, rows, cols, batch)
            assert tm['partial'] is True and tm['level'] == k
    t = C.read_region(path, planes=(2, 5), rows=(30, 34), cols=(1, 39), level=0, as_numpy=False)
    assert t.is_cuda and t.is_contiguous()
    assert np.array_equal(t.cpu().numpy().view(np.uint8), x[:, 2:5, 30:34, 1:39].view(np.uint8))
    for bad in ({'rows': (5, 5)}, {'cols': (9, 2)}, {'level': L + 1}, {'level': -1}, {'level': 1, 'rows': (17, 20)}):
        with pytest.raises(ValueError):
            C.read_region(path, **bad)


def test_planes_beyond_a_tile_default_threshold(kom, tmp_path):
    """Level 0's plane of cells is 132 * 132 = 17424 samples, more than a tile: rows are cropped there
    and the row runs begin and end in mid-tile; level 1's is 66 * 66: not cropped.

    The counts, by hand.  Every level-0 map is (1, 12, 132, 132, 1); a plane is 1.06 tiles, so the
    planes route's one range of 4 map planes touches 5 tiles, and a row run touches 1 unless a tile
    boundary falls inside it.  Planes (8, 16) are map planes 4 .. 7, whose tile boundaries (81920,
    98304, 114688, 131072) fall in map rows 92, 84, 76 and 68: rows (40, 80) -> map rows [20, 40)
    hold none, so the box reads 4 tiles per map where the planes route reads 5.  Planes (16, 24) are
    map planes 8 .. 11, the planes route reads tiles 8 .. 12; rows (224, 264) -> map rows [112, 132)
    lie in tiles 9, 10, 11 and 12: 4 of 5 again.  (A run a boundary does fall into -- rows (100, 140)
    of planes (8, 16), map row 68 of plane 7 -- touches 2 tiles and the box then reads as many tiles as
    the planes route: with planes this close to one tile the saving is one tile per array at most.)
    Level 1 and the coarsest lowres are read alike by both."""
    C = kom.container
    x = _field((1, 24, 264, 264, 1), np.uint16, seed=7)
    path = str(tmp_path / 'big.kmp')
    C.compress(path, x, kom.MeanPredictor(1, 3), levels=2)
    meta = C.load(path)[2]
    for planes, rows, cols in (((8, 16), (40, 80), (90, 130)), ((16, 24), (224, 264), (224, 264))):
        plan = C.plan_region(meta, planes=planes, rows=rows, cols=cols)
        l0, l1 = plan['levels']
        assert l0['rows']['local'] != (0, 132) and l1['rows']['local'] == (0, 66)
        assert any(f % TILE and e % TILE for ar in plan['arrays'][1:8] for f, e, _ in ar['ranges'])
        got = C.read_region(path, planes=planes, rows=rows, cols=cols)
        box = dict(C.last_timing)
        assert np.array_equal(got, x[:, planes[0]:planes[1], rows[0]:rows[1], cols[0]:cols[1]])
        slab = C.read_region(path, planes=planes)
        slab_tm = dict(C.last_timing)
        assert np.array_equal(slab[:, :, rows[0]:rows[1], cols[0]:cols[1]], got)
        assert box['tiles_decoded'] == plan['tiles_decoded'] and box['tiles_total'] == slab_tm['tiles_total']
        assert box['tiles_decoded'] == slab_tm['tiles_decoded'] - 7  # 4 of 5 tiles in each of level 0's 7 maps
        assert box['tiles_decoded'] < slab_tm['tiles_decoded']
        assert box['payload_bytes_read'] < slab_tm['payload_bytes_read']


@pytest.mark.parametrize('shape', [(1, 24, 36, 40, 1), (2, 21, 35, 41, 1)], ids=['even', 'odd'])
def test_level_reads(kom, tmp_path, shape):
    C = kom.container
    x = _field(shape, np.uint16, seed=shape[1])
    path = str(tmp_path / 'l.kmp')
    L = C.compress(path, x, kom.MeanPredictor(1, 3), levels=3)['levels']
    full = C.decompress(path)
    assert np.array_equal(C.read_region(path, level=1), full[:, ::2, ::2, ::2])
    assert C.last_timing['level'] == 1
    one = C.last_timing['tiles_decoded']
    assert np.array_equal(C.read_region(path, level=2), full[:, ::4, ::4, ::4])
    assert np.array_equal(C.read_region(path, level=0, rows=(3, 9)), full[:, :, 3:9])
    before = kom._lib.lib.kmp_last_launch().decode()
    assert before not in RICE_LAUNCHES and before  # the finest level's codec family ran last
    got = C.read_region(path, level=L)
    after = kom._lib.lib.kmp_last_launch().decode()
    assert np.array_equal(got, full[:, ::8, ::8, ::8]) and got.shape == C.level_shapes(path)[L]
    assert after in RICE_LAUNCHES  # nothing was launched after the ranged decode and its CRC: no codec kernel
    assert C.last_timing['tiles_decoded'] == 1 < one  # the coarsest lowres alone: one array within one tile
    for bad in (L + 1, -1):
        with pytest.raises(ValueError):
            C.read_region(path, level=bad)


def test_images(kom, tmp_path):
    C = kom.container
    rng = np.random.default_rng(0)
    img = (np.add.outer(np.arange(264), np.arange(300))[None, ..., None] // 3 +
           rng.integers(0, 4, (3, 264, 300, 1))).astype(np.uint8)
    path = str(tmp_path / 'i.kmp')
    L = C.compress(path, img, kom.MeanPredictor(1, 2), levels='auto')['levels']
    full = C.decompress(path)
    assert np.array_equal(full, img) and C.level_shapes(path)[0] == img.shape
    for k in (0, 1, L):
        want_k = full[:, ::2 ** k, ::2 ** k]
        H, W = want_k.shape[1:3]
        assert C.level_shapes(path)[k] == want_k.shape
        for rows in _axis_options(H):
            for cols, batch in zip(_axis_options(W), (None, (1, 3), (2, 3), None)):
                got = C.read_region(path, rows=rows, cols=cols, batch=batch, level=k)
                b = slice(*batch) if batch else slice(None)
                assert np.array_equal(got, want_k[b, rows[0]:rows[1], cols[0]:cols[1]]), (k, rows, cols, batch)
                assert C.last_timing['partial'] is True and got.flags['C_CONTIGUOUS']
    # a row band of one image: level 0's maps are (3, 132, 150, 1), two tiles per image, the band lies in the first
    C.read_region(path, rows=(100, 110), batch=(0, 1))
    band = C.last_timing['payload_bytes_read']
    C.read_region(path, batch=(0, 1))
    assert band < C.last_timing['payload_bytes_read']
    for kw in ({'planes': (0, 4)}, {'planes': (0, 4), 'rows': (0, 4)}):
        with pytest.raises(ValueError):
            C.read_region(path, **kw)


def test_tile_crc_covers_exactly_the_touched_tiles(kom, tmp_path):
    C = kom.container
    x = _field((1, 24, 264, 264, 1), np.uint16, seed=9)
    path = tmp_path / 'c.kmp'
    C.compress(str(path), x, kom.MeanPredictor(0, 3), levels=2, tile_crc=True)
    raw = bytearray(path.read_bytes())
    mlen = struct.unpack('<4sHHQ', bytes(raw[:16]))[3]
    base = 16 + mlen
    b = bytes(raw[base:])
    poff = struct.unpack('<Q', b[48:56])[0]
    meta = C.load(str(path))[2]
    sel = dict(planes=(8, 16), rows=(100, 140), cols=(90, 130))
    plan = C.plan_region(meta, **sel)
    ar = plan['arrays'][1]  # level 0's first map, (1, 12, 132, 132, 1): 13 tiles
    n, nb, nt, side, toff, first, end = struct.unpack('<5q2Q', b[80 + 128 + 72:80 + 256])
    tab = list(np.frombuffer(b, np.uint64, count=nt, offset=toff)) + [end]
    touched = {t for f, e, _ in ar['ranges'] for t in range(f // TILE, (e - 1) // TILE + 1)}
    assert nt == 13 and touched and len(touched) < nt
    near, far = min(touched), max(set(range(nt)) - touched)
    assert tab[near + 1] > tab[near] and tab[far + 1] > tab[far]

    def variant(name, tile):
        r = bytearray(raw)
        r[base + poff + 4 * int(tab[tile]) + 1] ^= 0x10
        (tmp_path / name).write_bytes(bytes(r))
        return str(tmp_path / name)

    want = x[:, 8:16, 100:140, 90:130]
    assert np.array_equal(C.read_region(str(path), **sel), want) and C.last_timing['tile_crc'] is True
    with pytest.raises(ValueError, match='tile CRC|side information'):
        C.read_region(variant('near.kmp', near), **sel)
    far_path = variant('far.kmp', far)
    assert np.array_equal(C.read_region(far_path, **sel), want) and C.last_timing['tile_crc'] is True
    with pytest.raises(ValueError):
        C.read_region(far_path, verify=True, **sel)
    # the damaged tile belongs to level 0: a read of level 1 does not touch it
    assert np.array_equal(C.read_region(variant('near1.kmp', near), level=1), x[:, ::2, ::2, ::2])


def test_fallback_files(kom, tmp_path, crop_everywhere):
    C = kom.container
    x = _field((1, 21, 34, 40, 1), np.uint16, seed=1)
    path = str(tmp_path / 'p.kmp')
    L = C.compress(path, x, kom.MeanPredictor(0, 3), method='planes', levels=2)['levels']
    assert C.level_shapes(path) == [(1, 21, 34, 40, 1), (1, 11, 17, 20, 1), (1, 6, 9, 10, 1)]
    assert np.array_equal(C.read_region(path, planes=(5, 12), rows=(3, 9), cols=(30, 99)), x[:, 5:12, 3:9, 30:40])
    assert C.last_timing['partial'] is False and C.last_timing['level'] == 0
    assert np.array_equal(C.read_region(path, rows=(3, 9), level=1), x[:, ::2, ::2, ::2][:, :, 3:9])
    assert np.array_equal(C.read_region(path, cols=(1, 4), level=L), x[:, ::4, ::4, ::4][:, :, :, 1:4])
    assert C.last_timing['partial'] is False and C.last_timing['level'] == L
    with pytest.raises(ValueError):
        C.read_region(path, level=L + 1)
    pred = kom.MeanPredictor(1, 3)
    lo, enc = kom.volume.encode(pred, kom.volume.encode_values_uint16, x, padding=1)
    spath = str(tmp_path / 's.kmp')
    C.save(spath, lo, enc, predictor=pred)  # a v2 Rice bundle of one level: the partial path
    assert C.level_shapes(spath) == [(1, 21, 34, 40, 1), (1, 11, 17, 20, 1)]
    assert np.array_equal(C.read_region(spath, planes=(5, 12), rows=(30, 34), cols=(0, 3)), x[:, 5:12, 30:34, 0:3])
    assert C.last_timing['partial'] is True
    assert np.array_equal(C.read_region(spath, rows=(2, 5), level=1), np.asarray(lo)[:, :, 2:5])
    assert C.last_timing['partial'] is True
    ppath = str(tmp_path / 'sp.kmp')
    C.save(ppath, lo, enc, predictor=pred, method='planes')
    assert np.array_equal(C.read_region(ppath, rows=(2, 5), cols=(7, 9), level=1), np.asarray(lo)[:, :, 2:5, 7:9])
    assert C.last_timing['partial'] is False


def test_opaque_predictions_fn(kom, tmp_path, crop_everywhere):
    C = kom.container
    x = _field((2, 21, 34, 40, 1), np.uint16, seed=2)
    inner = kom.MeanPredictor(1, 3)

    def my_predictor(lowres):
        return inner(lowres)

    lo, enc = kom.volume.encode(my_predictor, kom.volume.encode_values_uint16, x, padding=1)
    path = str(tmp_path / 'ext.kmp')
    C.save(path, lo, enc, predictor=my_predictor, padding=1)
    with pytest.raises(AssertionError, match='external'):
        C.read_region(path, rows=(5, 12))
    for planes, rows, cols in _boxes(x.shape)[::5]:
        got = C.read_region(path, planes=planes, rows=rows, cols=cols, batch=(1, 2), predictor=my_predictor)
        assert np.array_equal(got, x[1:2, planes[0]:planes[1], rows[0]:rows[1], cols[0]:cols[1]]), (planes, rows, cols)
        assert C.last_timing['partial'] is True
