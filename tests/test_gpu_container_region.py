"""container.read_region: planes / batch items of a compressed file, bit-equal to the slice of the
original array and of ``decompress(path)``, reading only the tiles the selection needs.

Volumes are ``[1, D, 20, 24, 1]`` (the trailing axis is the channel axis every codec entry point
asks for): D = 7 and 33 are odd (dims 0: the parity maps are a plane shorter), 34 and 64 even, 33 /
34 straddle a pyramid level whose depth changes parity, and every array is smaller than one tile,
so the multi-tile case has a test of its own."""

import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TILE = 16384


def _volume(shape, dtype, seed=0):
    """A smooth field plus noise (so the residuals are small but not zero), any dtype."""
    rng = np.random.default_rng(seed)
    g = np.indices(shape[1:4]).astype(np.float64)
    f = 60 * np.sin(g[0] / 5.0) + 40 * np.cos(g[1] / 3.0) + 30 * np.sin(g[2] / 4.0) + rng.normal(0, 2, shape[1:4])
    f = np.broadcast_to(f[None, ..., None], shape) + rng.normal(0, 1, shape)
    if dtype == np.float32:
        return f.astype(np.float32)
    return (np.rint(f + 200).astype(np.int64) % (1 << (8 * np.dtype(dtype).itemsize))).astype(dtype)


def _linear(kom, p, arith):
    n = (2 * p + 2) ** 3
    w = (np.full((n, 19), 1.0 / n) + np.random.default_rng(p).standard_normal((n, 19)) * 0.01).astype(np.float32)
    kw = {} if arith is None else {'arith': arith}
    return kom.LinearPredictor(w, np.zeros(19, np.float32), p, 3, **kw)


CONFIGS = [(f'{np.dtype(dt).name}-mean-p{p}', dt, ('mean', p, None)) for dt in (np.uint16, np.uint8) for p in (0, 1, 2)]
CONFIGS += [(f'u16-linear-p{p}-{a or "default"}', np.uint16, ('linear', p, a)) for p in (0, 1) for a in ('f32', None)]
CONFIGS += [('f32-mean-p0', np.float32, ('mean', 0, None))]


def _ranges(D):
    c = [(0, 1), (0, D), (D - 1, D), (D // 2, D // 2 + 1), (5, 12), (3, 6), (2, 7)]  # (3, 6) odd, (2, 7) even start
    return [(a, min(b, D)) for a, b in c if a < min(b, D)]


@pytest.mark.parametrize('levels', [1, 3, 'auto'])
@pytest.mark.parametrize('D', [7, 33, 34, 64])
@pytest.mark.parametrize('name,dtype,pred', CONFIGS, ids=[c[0] for c in CONFIGS])
def test_plane_ranges(kom, tmp_path, name, dtype, pred, D, levels):
    x = _volume((1, D, 20, 24, 1), dtype, seed=D)
    kind, p, arith = pred
    predictor = kom.MeanPredictor(p, 3) if kind == 'mean' else _linear(kom, p, arith)
    path = str(tmp_path / 'v.kmp')
    kom.container.compress(path, x, predictor, levels=levels)
    full = kom.container.decompress(path)
    assert np.array_equal(full.view(np.uint8), x.view(np.uint8))
    info = kom.container.info(path)
    assert info['shape'] == x.shape and info['sample_dtype'] == np.dtype(dtype).name
    for z0, z1 in _ranges(D):
        got = kom.container.read_region(path, planes=(z0, z1))
        assert kom.container.last_timing['partial'] is True
        assert got.dtype == x.dtype and got.shape == (1, z1 - z0, 20, 24, 1)
        assert np.array_equal(got.view(np.uint8), x[:, z0:z1].view(np.uint8)), f'{name} D={D} planes {(z0, z1)}'
        assert np.array_equal(got.view(np.uint8), full[:, z0:z1].view(np.uint8))
    t = kom.container.read_region(path, planes=(2, 5), as_numpy=False)
    assert t.is_cuda and np.array_equal(t.cpu().numpy().view(np.uint8), x[:, 2:5].view(np.uint8))


def test_batch_selections(kom, tmp_path):
    x = np.concatenate([_volume((1, 33, 20, 24, 1), np.uint16, seed=s) for s in range(3)])
    path = str(tmp_path / 'b.kmp')
    kom.container.compress(path, x, kom.MeanPredictor(1, 3))
    assert np.array_equal(kom.container.read_region(path, batch=(1, 3)), x[1:3])
    assert kom.container.last_timing['partial'] is True
    assert np.array_equal(kom.container.read_region(path, batch=(1, 3), planes=(4, 9)), x[1:3, 4:9])
    assert np.array_equal(kom.container.read_region(path, batch=(2, 99), planes=(-3, 2)), x[2:3, 0:2])  # clamped
    for bad in ({'batch': (2, 2)}, {'planes': (9, 4)}, {'batch': (3, 5)}):
        with pytest.raises(ValueError):
            kom.container.read_region(path, **bad)
    rng = np.random.default_rng(0)
    img = (np.add.outer(np.arange(40), np.arange(48))[None, ..., None] + rng.integers(0, 4, (6, 40, 48, 1))).astype(np.uint8)
    ipath = str(tmp_path / 'i.kmp')
    kom.container.compress(ipath, img, kom.MeanPredictor(0, 2))
    assert np.array_equal(kom.container.read_region(ipath, batch=(2, 5)), img[2:5])
    assert kom.container.last_timing['partial'] is True
    assert kom.container.info(ipath)['ndim'] == 2
    with pytest.raises(ValueError):
        kom.container.read_region(ipath, planes=(0, 4))


def _touched_tiles(path, kom, plan):
    """``(tiles, payload words)`` the plan's ranges touch, from the file's own tile tables."""
    raw = open(path, 'rb').read()
    mlen = struct.unpack('<4sHHQ', raw[:16])[3]
    b = raw[16 + mlen:]
    count = struct.unpack('<H', b[6:8])[0]
    tiles = words = 0
    for ar in plan['arrays']:
        r = b[80 + 128 * ar['index']:80 + 128 * (ar['index'] + 1)]
        n, nb, nt, side, toff, first, end = struct.unpack('<5q2Q', r[72:128])
        tab = list(np.frombuffer(b, np.uint64, count=nt, offset=toff)) + [end]
        for f, e, _ in ar['ranges']:
            t0, t1 = f // TILE, (e - 1) // TILE
            tiles += t1 - t0 + 1
            words += int(tab[t1 + 1]) - int(tab[t0])
    assert count == len(plan['arrays'])
    return tiles, words


def test_multi_tile_volume_reads_a_fraction(kom, tmp_path):
    shape = (1, 40, 128, 128, 1)
    x = _volume(shape, np.uint16, seed=3)
    path = str(tmp_path / 'm.kmp')
    kom.container.compress(path, x, kom.MeanPredictor(1, 3), levels=2)
    got = kom.container.read_region(path, planes=(18, 22))
    tm = dict(kom.container.last_timing)
    assert np.array_equal(got, x[:, 18:22])
    # the count from the shapes (every extent is even, so all 7 maps of a level have the lowres's
    # shape): level 0 needs planes [9, 11) of 7 maps [20, 64, 64], level 1 planes [3, 7) of 7 maps
    # [10, 32, 32], and the coarsest lowres [10, 32, 32] planes [1, 9)
    def tiles_of(z0, z1, h, w):
        return (z1 * h * w - 1) // TILE - (z0 * h * w) // TILE + 1
    want = 7 * tiles_of(9, 11, 64, 64) + 7 * tiles_of(3, 7, 32, 32) + tiles_of(1, 9, 32, 32)
    total = 7 * -(-20 * 64 * 64 // TILE) + 7 * -(-10 * 32 * 32 // TILE) + -(-10 * 32 * 32 // TILE)
    assert (want, total) == (15, 43)
    assert tm['partial'] is True and tm['tiles_decoded'] == want and tm['tiles_total'] == total
    assert tm['tiles_decoded'] < tm['tiles_total'] and 2 * tm['tiles_decoded'] <= tm['tiles_total']
    meta = kom.container.load(path)[2]
    tiles, words = _touched_tiles(path, kom, kom.container.plan_region(meta, (18, 22)))
    assert tiles == want and tm['payload_bytes_read'] == 4 * words
    assert tm['bundle_bytes'] == meta['bundle_bytes']


def test_fallback_and_save_files(kom, tmp_path):
    x = _volume((1, 33, 20, 24, 1), np.uint16, seed=1)
    path = str(tmp_path / 'p.kmp')
    kom.container.compress(path, x, kom.MeanPredictor(0, 3), method='planes')
    assert np.array_equal(kom.container.read_region(path, planes=(5, 12)), x[:, 5:12])
    assert kom.container.last_timing['partial'] is False
    pred = kom.MeanPredictor(1, 3)
    lo, enc = kom.volume.encode(pred, kom.volume.encode_values_uint16, x, padding=1)
    spath = str(tmp_path / 's.kmp')
    kom.container.save(spath, lo, enc, predictor=pred)
    assert np.array_equal(kom.container.read_region(spath, planes=(5, 12)), x[:, 5:12])
    assert kom.container.last_timing['partial'] is True


def test_integrity(kom, tmp_path):
    shape = (1, 40, 128, 128, 1)
    x = _volume(shape, np.uint16, seed=4)
    path = tmp_path / 'g.kmp'
    kom.container.compress(str(path), x, kom.MeanPredictor(1, 3), levels=2)
    raw = bytearray(path.read_bytes())
    mlen = struct.unpack('<4sHHQ', bytes(raw[:16]))[3]
    base = 16 + mlen
    b = bytes(raw[base:])
    poff = struct.unpack('<Q', b[48:56])[0]
    # array 1 = level 0's first map [1, 20, 64, 64, 1]: planes [9, 11) are samples 36864 .. 45055, tile 2 of 5
    n, nb, nt, side, toff, first, end = struct.unpack('<5q2Q', b[80 + 128 + 72:80 + 256])
    tab = np.frombuffer(b, np.uint64, count=nt, offset=toff)
    assert nt == 5 and (9 * 64 * 64) // TILE == 2 and (11 * 64 * 64 - 1) // TILE == 2
    bw_off = side + (nb + 7) // 8 * 8

    def variant(name, at, flip=1):
        r = bytearray(raw)
        r[at] ^= flip
        p = tmp_path / name
        p.write_bytes(bytes(r))
        return str(p)

    # a payload byte of tile 4 (untouched): not noticed without verify, the CRC catches it with
    far = variant('far.kmp', base + poff + 4 * int(tab[4]) + 1, 0x10)
    assert np.array_equal(kom.container.read_region(far, planes=(18, 22)), x[:, 18:22])
    with pytest.raises(ValueError):
        kom.container.read_region(far, planes=(18, 22), verify=True)
    with pytest.raises(ValueError):
        kom.container.decompress(far)
    # a bw byte of tile 2 (touched): the decode's own check, either way
    near = variant('near.kmp', base + bw_off + 2 * 256 + 5)
    for verify in (False, True):
        with pytest.raises(ValueError):
            kom.container.read_region(near, planes=(18, 22), verify=verify)
    # a truncated file, and a table entry past the payload
    (tmp_path / 'trunc.kmp').write_bytes(bytes(raw[:-100]))
    with pytest.raises(ValueError):
        kom.container.read_region(str(tmp_path / 'trunc.kmp'), planes=(18, 22))
    r = bytearray(raw)
    r[base + toff + 8 * 3:base + toff + 8 * 4] = struct.pack('<Q', 1 << 40)  # tile 3 = the closing entry of tile 2
    (tmp_path / 'table.kmp').write_bytes(bytes(r))
    with pytest.raises(ValueError):
        kom.container.read_region(str(tmp_path / 'table.kmp'), planes=(18, 22))
    assert np.array_equal(kom.container.read_region(str(path), planes=(18, 22), verify=True), x[:, 18:22])


def test_predictor_checks_match_decompress(kom, tmp_path):
    x = _volume((2, 33, 20, 24, 1), np.uint16, seed=2)
    inner = kom.MeanPredictor(0, 3)

    def my_predictor(lowres):
        return inner(lowres)

    lo, enc = kom.volume.encode(my_predictor, kom.volume.encode_values_uint16, x)
    path = str(tmp_path / 'ext.kmp')
    kom.container.save(path, lo, enc, predictor=my_predictor)
    with pytest.raises(AssertionError, match='external'):
        kom.container.read_region(path, planes=(5, 12))
    assert np.array_equal(kom.container.read_region(path, planes=(5, 12), predictor=inner), x[:, 5:12])
    assert np.array_equal(kom.container.read_region(path, planes=(5, 12), batch=(1, 2), predictor=my_predictor),
                          x[1:2, 5:12])
    rng = np.random.default_rng(3)
    w = (rng.standard_normal((8, 19)) / 8).astype(np.float32)
    b = np.zeros(19, np.float32)
    for enc_a, dec_a in (('bf16x2', 'f32'), ('f32', 'bf16x2')):
        path = str(tmp_path / f'{enc_a}.kmp')
        kom.container.compress(path, x, kom.LinearPredictor(w, b, 0, 3, arith=enc_a))
        assert np.array_equal(kom.container.read_region(path, planes=(5, 12)), x[:, 5:12])
        assert np.array_equal(kom.container.read_region(path, planes=(5, 12), predictor=kom.LinearPredictor(w, b, 0, 3)),
                              x[:, 5:12])
        with pytest.raises(AssertionError):
            kom.container.read_region(path, planes=(5, 12), predictor=kom.LinearPredictor(w, b, 0, 3, arith=dec_a))
    with pytest.raises(AssertionError, match='padding'):
        kom.container.read_region(path, planes=(5, 12), predictor=kom.MeanPredictor(1, 3))
