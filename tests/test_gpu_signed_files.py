"""Signed samples (int8 / int16) through the packers, the container, the tile stream and the captured
codec plans.  Data: tests/signed_spec.py (zero-crossing field, full-range noise, the extremes)."""

import numpy as np
import pytest
import torch

import signed_spec as S

pytestmark = pytest.mark.gpu

I8, I16 = np.int8, np.int16
DTYPES = [I16, I8]
IDS = ['int16', 'int8']


@pytest.mark.parametrize('method', ['rice', 'planes'])
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_pack_unpack_keep_the_dtype(kom, dtype, method):
    P = kom.packing
    for shape in ((3, 7, 33), (20000,), (5,)):
        x = S.uniform(shape, dtype, seed=len(shape))
        x.reshape(-1)[:5] = S.extremes(dtype)
        blob = P.pack(x, method)
        back = P.unpack(blob)
        assert back.dtype == np.dtype(dtype) and back.shape == x.shape and np.array_equal(back, x)
    # small signed values stay small under the Rice zigzag: a signed array packs like its bit pattern
    small = S.zero_crossing((1, 16, 16, 16, 1), dtype, seed=2)
    assert len(P.pack(small, method)) == len(P.pack(small.view(S.unsigned_of(dtype)), method))
    t = torch.from_numpy(small).cuda()
    assert torch.equal(P.unpack(P.pack(t, method)), t)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_pack_encoded_round_trip_and_ranges(kom, dtype):
    P, V = kom.packing, kom.volume
    x = S.data((2, 12, 16, 64, 1), dtype, seed=4)
    name = np.dtype(dtype).name
    lo, (maps, dims) = V.encode(kom.MeanPredictor(0, 3), getattr(V, 'encode_values_' + name), x)
    blob = P.pack_encoded(lo, (maps, dims))
    lo2, (maps2, dims2) = P.unpack_encoded(blob)
    assert lo2.dtype == np.dtype(dtype) and np.array_equal(lo2, lo) and tuple(dims2) == tuple(dims)
    for a, b in zip(maps, maps2):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    got = P.unpack_ranges(blob, [(0, 3, lo.size - 2), (1, 0, 7)])
    assert got[0].dtype == np.dtype(dtype) and np.array_equal(got[0], lo.reshape(-1)[3:lo.size - 2])
    assert np.array_equal(got[1], maps[0].reshape(-1)[:7])


@pytest.mark.parametrize('tile_crc', [False, True])
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_container_round_trip_region_check_info(kom, tmp_path, dtype, tile_crc):
    C = kom.container
    x = S.data((2, 40, 24, 32, 1), dtype, seed=7)
    path = str(tmp_path / 'signed.kmp')
    stats = C.compress(path, x, kom.MeanPredictor(0, 3), levels=2, tile_crc=tile_crc)
    assert stats['levels'] == 2
    info = C.info(path)
    assert info['sample_dtype'] == np.dtype(dtype).name and info['shape'] == x.shape and info['levels'] == 2
    assert ('tile_crc' in info) == tile_crc
    back = C.decompress(path)
    assert back.dtype == np.dtype(dtype) and np.array_equal(back, x)
    # planes [13, 29) straddle an output-plane pair of both levels; batch item 1 only
    part = C.read_region(path, planes=(13, 29), batch=(1, 2))
    assert part.dtype == np.dtype(dtype) and np.array_equal(part, x[1:2, 13:29])
    assert C.last_timing['partial'] is True and C.last_timing['tile_crc'] == tile_crc
    assert np.array_equal(C.read_region(path, planes=(0, 40)), x)
    chk = C.check(path)
    assert chk['ok'] and chk['crc32'] and ((chk['tile_crc'] is not None) == tile_crc)
    # the coarsest lowres travels as the signed samples themselves, under the signed dtype
    lo, (maps, _), meta = C.load(path, device=False)
    assert lo.dtype == np.dtype(dtype) and np.array_equal(lo, x[:, ::4, ::4, ::4])
    assert meta['sample_dtype'] == np.dtype(dtype).name and all(m.dtype == S.unsigned_of(dtype) for m in maps)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_linear_predictor_file_and_save_load(kom, tmp_path, dtype):
    C, V = kom.container, kom.volume
    x = S.data((1, 17, 18, 20, 1), dtype, seed=1)
    lin = kom.LinearPredictor(*S.clamp_weights(8, 19), 0, 3)
    path = str(tmp_path / 'lin.kmp')
    C.compress(path, x, lin, levels=1)
    assert np.array_equal(C.decompress(path), x)          # the file's own predictor ('f32' recorded)
    assert np.array_equal(C.decompress(path, lin), x)     # a default-constructed one takes the file's
    name = np.dtype(dtype).name
    pred = kom.MeanPredictor(1, 3)
    lo, enc = V.encode(pred, getattr(V, 'encode_values_' + name), x, padding=1)
    path2 = str(tmp_path / 'saved.kmp')
    C.save(path2, lo, enc, predictor=pred)
    assert C.info(path2)['sample_dtype'] == name
    lo2, (maps2, dims2), _ = C.load(path2, device=False)
    assert lo2.dtype == np.dtype(dtype) and np.array_equal(lo2, lo)
    assert np.array_equal(C.decompress(path2), x)


def test_signed_file_differs_from_the_shifted_unsigned_file_in_lowres_and_metadata_only(kom, tmp_path):
    C = kom.container
    x = S.data((1, 24, 16, 32, 1), I16, seed=3)
    u = S.M(x)  # x + 32768 as uint16
    ps, pu = str(tmp_path / 's.kmp'), str(tmp_path / 'u.kmp')
    C.compress(ps, x, kom.MeanPredictor(0, 3), levels=2)
    C.compress(pu, u, kom.MeanPredictor(0, 3), levels=2)
    los, (ms, ds), metas = C.load(ps, device=False)
    lou, (mu, du), metau = C.load(pu, device=False)
    assert tuple(ds) == tuple(du) and len(ms) == len(mu) == 14
    for a, b in zip(ms, mu):
        assert a.dtype == b.dtype == np.uint16 and np.array_equal(a, b)
    assert los.dtype == np.int16 and lou.dtype == np.uint16 and np.array_equal(S.M(los), lou)
    volatile = ('sample_dtype', 'bundle_bytes', 'crc32')
    assert {k: v for k, v in metas.items() if k not in volatile} == {k: v for k, v in metau.items() if k not in volatile}
    assert (metas['sample_dtype'], metau['sample_dtype']) == ('int16', 'uint16')
    # the signed lowres (values near zero under the Rice zigzag) codes no larger than the shifted one
    assert len(kom.packing.pack(los)) <= len(kom.packing.pack(lou))


def test_existing_dtypes_keep_their_file_bytes(kom, tmp_path):
    """The dtype code and the metadata of an unsigned file are what they were: code 1 in the bundle's
    array records, 'uint16' in the metadata, no signed field anywhere."""
    C = kom.container
    u = S.M(S.data((1, 16, 16, 32, 1), I16, seed=5))
    path = str(tmp_path / 'u.kmp')
    C.compress(path, u, kom.MeanPredictor(0, 3), levels=1)
    lo, (maps, dims), meta = C.load(path)
    assert sorted(meta) == sorted(['format', 'ndim', 'padding', 'method', 'sample_dtype', 'levels', 'lowres_shape',
                                   'predictor', 'bundle_bytes', 'crc32'])
    blob = kom.packing.pack_encoded(lo, (maps, ()))
    recs = [int.from_bytes(bytes(blob[80 + 128 * i:84 + 128 * i].cpu().numpy()), 'little') for i in range(8)]
    assert recs == [1] * 8


@pytest.mark.parametrize('bad', ['int64', 'sint6'])
def test_unknown_sample_dtype_is_refused(kom, tmp_path, bad):
    C = kom.container
    x = S.data((1, 12, 16, 32, 1), I16, seed=2)
    path = str(tmp_path / 'x.kmp')
    C.compress(path, x, kom.MeanPredictor(0, 3), levels=1)
    raw = open(path, 'rb').read()
    key = b'"sample_dtype":"int16"'
    assert raw.count(key) == 1
    open(path, 'wb').write(raw.replace(key, b'"sample_dtype":"%s"' % bad.encode()))
    for call in (C.decompress, C.info, C.load, C.check, lambda p: C.read_region(p, planes=(0, 4))):
        with pytest.raises(ValueError, match='sample dtype'):
            call(path)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('zero_copy', [False, True])
def test_tile_stream(kom, dtype, zero_copy):
    shape, chunk, slots = (10, 16, 16, 16, 1), 3, 2  # the smallest shape of test_gpu_stream.py, ragged last chunk
    x = S.data(shape, dtype, seed=11)
    V = kom.volume
    pred = kom.MeanPredictor(0, 3)
    name = np.dtype(dtype).name
    ref_lo, (ref_maps, _) = V.encode(pred, getattr(V, 'encode_values_' + name), torch.from_numpy(x).cuda())
    ts = kom.stream.TileStream(pred, shape[1:], torch.from_numpy(x[:0]).dtype, chunk, slots, 3, zero_copy=zero_copy)
    src = torch.empty(x.shape, dtype=torch.from_numpy(x[:0]).dtype, pin_memory=True)
    src.copy_(torch.from_numpy(x))
    lo, maps = ts.alloc_encoded(shape[0])
    ts.encode(src, lo, maps)
    ts.synchronize()
    assert lo.dtype == src.dtype and torch.equal(lo, ref_lo.cpu())
    assert all(torch.equal(a, b.cpu()) for a, b in zip(maps, ref_maps))
    out = torch.empty_like(src).pin_memory()
    ts.decode(lo, maps, out)
    ts.synchronize()
    assert torch.equal(out, src)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_codec_plan(kom, dtype):
    shape = (4, 32, 32, 32, 1)  # the smallest shape of test_gpu_graphs.py
    V = kom.volume
    name = np.dtype(dtype).name
    enc, dec = getattr(V, 'encode_values_' + name), getattr(V, 'decode_values_' + name)
    pred = kom.MeanPredictor(0, 3)
    td = torch.from_numpy(np.zeros(0, dtype)).dtype
    plan = kom.graphs.CodecPlan(pred, shape, td)
    for rep in range(2):
        x = torch.from_numpy(S.data(shape, dtype, seed=rep)).cuda()
        lo, (maps, dims) = plan.encode(x)
        want_lo, (want_maps, want_dims) = V.encode(pred, enc, x, padding=0)
        assert lo.dtype == td and torch.equal(lo, want_lo) and tuple(dims) == tuple(want_dims)
        assert all(torch.equal(a, b) for a, b in zip(maps, want_maps))
        assert torch.equal(plan.decode(), x)
        assert torch.equal(V.decode(pred, dec, lo, (maps, dims), padding=0), x)
