"""Per-tile CRCs, on the CPU: the specification helper (tests/tile_crc_spec.py) against a second
derivation from ``oracle.rice.pack``'s arrays and a bit-at-a-time CRC, and the container's pure host
functions (global tile index, trailer validation, ``info``)."""

import json
import struct
import zlib

import numpy as np
import pytest

from oracle import rice as R
from kompressor_amd import container, packing, _nd

import tile_crc_spec as S


def _residuals(n, dtype, seed, scale):
    rng = np.random.default_rng(seed)
    if scale is None:  # full-range noise
        info = np.iinfo(dtype)
        return rng.integers(info.min, int(info.max) + 1, size=n, dtype=np.int64).astype(dtype)
    return np.rint(rng.laplace(0, scale, n)).astype(np.int64).astype(dtype)


def _from_arrays(arrays):
    """The table from ``oracle.rice.pack``'s per-array (params, bw, payload): no bundle bytes parsed."""
    out = []
    for a in arrays:
        params, bw, payload = R.pack(a.reshape(-1))
        off = np.concatenate([[0], np.cumsum(bw.astype(np.int64))])
        for t in range(S.tiles_of(a.size)):
            b0, b1 = 256 * t, min(256 * (t + 1), len(params))
            data = params[b0:b1].tobytes() + bw[b0:b1].tobytes() + \
                payload[off[b0]:off[b1]].astype('<u4').tobytes()
            out.append(zlib.crc32(data) & 0xffffffff)
    return np.array(out, np.uint32)


def test_spec_on_mixed_dtypes():
    arrays = [_residuals(16385, np.uint8, 0, 3.0).reshape(1, 16385), np.zeros(700, np.uint16),
              _residuals(40000, np.uint16, 1, 40.0).reshape(2, 20000), _residuals(20000, np.int32, 2, None),
              _residuals(5000, np.uint32, 3, 1000.0)]
    b = R.pack_bundle(arrays)
    table = S.tile_crc_table(b)
    assert table.dtype == np.uint32 and len(table) == sum(S.tiles_of(a.size) for a in arrays) == 2 + 1 + 3 + 2 + 1
    assert np.array_equal(table, _from_arrays(arrays))
    assert S.tile_begin(b) == [0, 2, 3, 6, 8]
    # an all-zero tile has no payload words: the CRC of its side bytes alone
    assert table[2] == zlib.crc32(bytes(2 * 11))
    for a, t in ((0, 1), (2, 2), (3, 0)):  # a 1-block last tile, a short last tile, a near-maximal tile
        data = S.tile_bytes(b, a, t)
        assert S.crc32_bitwise(data) == table[S.tile_begin(b)[a] + t]
    assert len(S.tile_bytes(b, 0, 1)) == 2 + 4 * int(b[S.bundle_arrays(b)[0][0]['bw'] + 256])


@pytest.mark.parametrize('n', [1, 64, 65, 16383, 16384, 16385])
def test_spec_tile_edges(n):
    arrays = [_residuals(n, np.uint16, n, 25.0), _residuals(n, np.uint8, n + 1, 2.0)]
    b = R.pack_bundle(arrays)
    table = S.tile_crc_table(b)
    assert len(table) == 2 * S.tiles_of(n) == 2 * (2 if n > 16384 else 1)
    assert np.array_equal(table, _from_arrays(arrays))
    recs, poff = S.bundle_arrays(b)
    last = S.tiles_of(n) - 1
    nbk = -(-n // 64) - 256 * last
    data = S.tile_bytes(b, 1, last)
    closing = recs[1]['end']
    start = struct.unpack('<Q', b.tobytes()[recs[1]['toff'] + 8 * last:recs[1]['toff'] + 8 * last + 8])[0]
    assert len(data) == 2 * nbk + 4 * (closing - start)
    assert S.crc32_bitwise(data) == table[-1]


def test_global_tile_index_against_brute_force():
    rng = np.random.default_rng(5)
    ns = [int(v) for v in rng.integers(0, 70000, 40)] + [0, 1, 16384, 16385]
    counts = [S.tiles_of(n) for n in ns]
    brute = {}
    g = 0
    for a, c in enumerate(counts):
        for t in range(c):
            brute[(a, t)] = g
            g += 1
    begins = container._tile_begins(counts)
    pb, total = packing.tile_begins(ns)
    assert begins == pb and total == g
    assert all(begins[a] + t == v for (a, t), v in brute.items())
    assert [container._tiles(n) for n in ns] == counts == [packing._tiles_of(n) for n in ns]


def _meta(shape, levels, p):
    lv, s = [], tuple(shape)
    for _ in range(levels):
        lo, _, dims = _nd.encoded_shapes(s, 3)
        lv.append({'highres_shape': list(s), 'dims': [int(d) for d in dims]})
        s = tuple(lo)
    return {'format': 'kompressor_amd', 'ndim': 3, 'padding': p, 'method': 'rice', 'sample_dtype': 'uint16',
            'levels': lv, 'lowres_shape': list(s), 'predictor': {'kind': 'mean', 'padding': p, 'ndim': 3}}


def test_meta_tile_counts():
    meta = _meta((1, 40, 128, 128, 1), 2, 1)
    counts = container._meta_tile_counts(meta)
    assert len(counts) == 15 and sum(counts) == 43 == container.plan_region(meta)['tiles_total']
    assert counts[0] == 1 and counts[1] == 5
    # B = 2: every array is twice as long (tiles do not restart per batch item)
    assert sum(container._meta_tile_counts(_meta((2, 40, 128, 128, 1), 2, 1))) == \
        container.plan_region(_meta((2, 40, 128, 128, 1), 2, 1), batch=(0, 2))['tiles_total']


def test_trailer_validation():
    meta = _meta((1, 40, 128, 128, 1), 2, 1)
    n = 1000
    assert container._tile_crc_trailer(meta, n, n) is None
    good = dict(meta, tile_crc={'offset': 1000, 'tiles': 43})
    assert container._tile_crc_trailer(good, n, n + 4 * 43) == (1000, 43)
    assert container._tile_crc_trailer(dict(meta, tile_crc={'offset': 1008, 'tiles': 43}), 1001, 1008 + 4 * 43) == \
        (1008, 43)
    for bad, avail in ((dict(meta, tile_crc={'offset': 992, 'tiles': 43}), 4000),     # inside the bundle
                       (dict(meta, tile_crc={'offset': 1 << 50, 'tiles': 43}), 4000),  # far outside
                       (dict(meta, tile_crc={'offset': 1000, 'tiles': 42}), 4000),     # count
                       (dict(meta, tile_crc={'offset': 1000, 'tiles': 1 << 40}), 4000),
                       (good, n + 4 * 43 - 1),                                         # truncated
                       (dict(meta, tile_crc={'offset': 1000}), 4000),
                       (dict(meta, tile_crc=[1000, 43]), 4000),
                       (dict(meta, tile_crc={'offset': '1000', 'tiles': 43}), 4000),
                       (dict(good, method='planes'), 4000)):
        with pytest.raises(ValueError):
            container._tile_crc_trailer(bad, n, avail)


def _hand_file(tmp_path, name, with_table):
    import oracle
    from oracle import predictors as OP
    rng = np.random.default_rng(21)
    vol = rng.integers(0, 4096, (1, 21, 9, 10, 1)).astype(np.uint16)
    x, per = vol, []
    for _ in range(2):
        x, (maps, dims) = oracle.volume.encode(OP.mean_predictions_fn(1, 3), oracle.volume.encode_values_uint16, x,
                                               padding=1)
        per.append(maps)
    bundle = R.pack_bundle([np.asarray(x)] + [np.asarray(m) for maps in per for m in maps]).tobytes()
    meta = dict(_meta(vol.shape, 2, 1), bundle_bytes=len(bundle), crc32=zlib.crc32(bundle))
    trailer = b''
    if with_table:
        table = S.tile_crc_table(bundle)
        meta['tile_crc'] = {'offset': len(bundle) + (-len(bundle) % 8), 'tiles': len(table)}
        trailer = bytes(-len(bundle) % 8) + table.astype('<u4').tobytes()
    js = json.dumps(meta).encode()
    js += b' ' * (-len(js) % 8)
    path = tmp_path / name
    path.write_bytes(struct.pack('<4sHHQ', b'KMPF', 3, 0, len(js)) + js + bundle + trailer)
    return path, len(js), len(bundle), len(trailer)


def test_info_reports_a_table_only_where_there_is_one(tmp_path):
    path, mlen, nb, nt = _hand_file(tmp_path, 'table.kmp', True)
    plain, pm, pb, _ = _hand_file(tmp_path, 'plain.kmp', False)
    want = {'shape': (1, 21, 9, 10, 1), 'sample_dtype': 'uint16', 'ndim': 3, 'levels': 2, 'padding': 1,
            'predictor': 'mean', 'method': 'rice', 'version': 3, 'file_bytes': 16 + pm + pb, 'bundle_bytes': pb}
    assert container.info(str(plain)) == want  # exactly the keys a file without a table always had
    got = container.info(str(path))
    assert got == dict(want, file_bytes=16 + mlen + nb + nt, tile_crc=15)  # 15 arrays of one tile each
    (tmp_path / 'short.kmp').write_bytes(path.read_bytes()[:-1])
    with pytest.raises(ValueError):
        container.info(str(tmp_path / 'short.kmp'))
