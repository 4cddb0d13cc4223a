"""Per-tile CRCs (kmp_rice_tile_crc, packing.tile_crcs, the container's ``tile_crc`` trailer).

The expected values come from tests/tile_crc_spec.py: ``zlib.crc32`` over the documented byte
layout of a bundle.  Kernel shapes: an all-zero u8 array of 16385 samples (tiles without payload
words, a 1-block last tile), u16 byte-range residuals of 3 tiles + 100 samples, int32 full-range
noise of 2 tiles + 100 samples (tiles near the 67584-byte maximum: 66 wave steps, spans of many
alignments) and u16 arrays of 1 and 63 samples.  Files: the 43-tile geometry of
test_gpu_container_region.py::test_integrity, where planes (18, 22) touch tile 2 of array 1."""

import json
import re
import struct

import numpy as np
import pytest
import torch

import guard_spec as G
import tile_crc_spec as S

pytestmark = pytest.mark.gpu

TILE = 16384
MAX_SPAN = 256 * (2 * 32 + 2)


# ---------------------------------------------------------------------------------------------
# the kernel
# ---------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def bundle(kom):
    """``(bundle bytes (numpy), resident bundle (device), the spec's table, parsed records, payload offset)``."""
    rng = np.random.default_rng(77)
    arrs = [np.zeros(16385, np.uint8),
            rng.integers(0, 256, 3 * TILE + 100).astype(np.uint16),
            rng.integers(-(1 << 31), 1 << 31, 2 * TILE + 100, dtype=np.int64).astype(np.int32),
            rng.integers(0, 256, 1).astype(np.uint16),
            rng.integers(0, 256, 63).astype(np.uint16)]
    blob = kom.packing.pack_encoded(arrs[0], (tuple(arrs[1:]), ()))
    recs, poff = S.bundle_arrays(blob)
    table = S.tile_crc_table(blob)
    assert len(table) == 2 + 4 + 3 + 1 + 1
    return blob, torch.from_numpy(blob).cuda(), table, recs, poff


def test_table_matches_the_spec(kom, bundle):
    blob, dblob, table, recs, poff = bundle
    got = kom.packing.tile_crcs(blob)  # numpy in -> numpy out
    assert kom._lib.lib.kmp_last_launch() == b'rice_tile_crc'
    assert isinstance(got, np.ndarray) and got.dtype == np.uint32
    assert np.array_equal(got, table), [hex(v) for v in got ^ table]
    dgot = kom.packing.tile_crcs(dblob)
    assert isinstance(dgot, torch.Tensor) and dgot.is_cuda and dgot.dtype == torch.uint32
    assert np.array_equal(dgot.view(torch.int32).cpu().numpy().view(np.uint32), table)
    # the int32 noise tiles are near the maximum span; the zero array's tiles have no payload words
    b = blob.tobytes()
    tab2 = struct.unpack('<3Q', b[recs[2]['toff']:recs[2]['toff'] + 24])
    assert tab2[1] - tab2[0] > MAX_SPAN - 512
    assert recs[0]['first'] == recs[0]['end']


def test_planes_blob_has_no_tiles(kom):
    blob = kom.packing.pack(np.arange(1000, dtype=np.uint16), method='planes')
    with pytest.raises(ValueError):
        kom.packing.tile_crcs(blob)


def _windows(bundle, ranges, misalign=0):
    """A device buffer holding, for each ``(array, t0, t1)``, only the touched tiles' table entries,
    the closing word (apart from them), the side bytes and the payload words; returns the buffer and
    per range the byte offsets ``(toff, closing, params, bw, payload, payload_first, payload_words)``.
    The payload windows start ``4 * (misalign + index)`` bytes past an 8-byte boundary."""
    blob, dblob, table, recs, poff = bundle
    b = blob.tobytes()
    parts, offs, at = [], [], 0

    def put(data, align, skew=0):
        nonlocal at
        pad = (-at) % align + skew
        parts.append(bytes([0xEE]) * pad + data)
        at += pad + len(data)
        return at - len(data)

    for q, (a, t0, t1) in enumerate(ranges):
        r = recs[a]
        cnt = t1 - t0 + 1
        tab = list(struct.unpack(f'<{r["nt"]}Q', b[r['toff']:r['toff'] + 8 * r['nt']])) + [r['end']]
        o_t = put(struct.pack(f'<{cnt}Q', *tab[t0:t1 + 1]), 8)
        nside = min(r['nb'], 256 * (t1 + 1)) - 256 * t0
        o_p = put(b[r['side'] + 256 * t0:r['side'] + 256 * t0 + nside], 1, 3)
        o_b = put(b[r['bw'] + 256 * t0:r['bw'] + 256 * t0 + nside], 1, 1)
        o_c = put(struct.pack('<Q', tab[t1 + 1]), 8)
        w0, w1 = tab[t0], tab[t1 + 1]
        o_w = put(b[poff + 4 * w0:poff + 4 * w1], 8, 4 * ((misalign + q) % 4))
        offs.append((o_t, o_c, o_p, o_b, o_w, w0, w1 - w0))
    buf = torch.from_numpy(np.frombuffer(b''.join(parts) + bytes(16), np.uint8).copy()).cuda()
    assert buf.data_ptr() % 8 == 0
    return buf, offs


RANGES = [(0, 0, 1), (0, 1, 1), (1, 0, 3), (1, 1, 2), (1, 3, 3), (2, 0, 2), (2, 1, 1), (2, 2, 2), (3, 0, 0), (4, 0, 0)]


@pytest.mark.parametrize('misalign', [0, 1, 2, 3])
def test_windows_give_the_same_values_and_write_nothing_else(kom, bundle, misalign):
    blob, dblob, table, recs, poff = bundle
    begins = S.tile_begin(blob)
    buf, offs = _windows(bundle, RANGES, misalign)
    wp = buf.data_ptr()
    for sentinel in G.SENTINELS:
        outs, records = [], []
        for q, ((a, t0, t1), (o_t, o_c, o_p, o_b, o_w, w0, pw)) in enumerate(zip(RANGES, offs)):
            c = G.carve_arena((t1 - t0 + 1,), torch.int32, 'cuda', sentinel, shift=4 * (q % 3))
            outs.append(c)
            records.append((recs[a]['n'], t0, t1, wp + o_p, wp + o_b, wp + o_t, wp + o_c, wp + o_w, w0, pw,
                            c.payload.data_ptr(), None))
        bad = torch.zeros((1,), dtype=torch.int64, device='cuda')
        assert kom.packing._launch_tile_crc(records, bad) == sum(t1 - t0 + 1 for _, t0, t1 in RANGES)
        assert int(bad.item()) == 0
        for (a, t0, t1), c in zip(RANGES, outs):
            arena = c.arena_bytes()
            lo = G.GUARD + c.shift
            assert (arena[:lo] == sentinel).all() and (arena[lo + c.nbytes:] == sentinel).all(), (a, t0, t1)
            got = arena[lo:lo + c.nbytes].view(np.uint32)
            assert np.array_equal(got, table[begins[a] + t0:begins[a] + t1 + 1]), (a, t0, t1)


def test_expect_mode_counts_exactly_the_perturbed_entries(kom, bundle):
    blob, dblob, table, recs, poff = bundle
    begins = S.tile_begin(blob)
    buf, offs = _windows(bundle, RANGES)
    wp = buf.data_ptr()
    for perturb in ([], [(3, 1)], [(0, 0), (2, 1), (5, 2), (9, 0)]):  # (range index, tile within it)
        exps, records = [], []
        for q, ((a, t0, t1), (o_t, o_c, o_p, o_b, o_w, w0, pw)) in enumerate(zip(RANGES, offs)):
            e = table[begins[a] + t0:begins[a] + t1 + 1].copy()
            for pq, pt in perturb:
                if pq == q:
                    e[pt] ^= np.uint32(1 << (7 * pt + 3))
            c = G.carve_arena((t1 - t0 + 1,), torch.int32, 'cuda', 0xA5)
            G.fill(c, e.view(np.int32))
            exps.append((c, e))
            records.append((recs[a]['n'], t0, t1, wp + o_p, wp + o_b, wp + o_t, wp + o_c, wp + o_w, w0, pw,
                            None, c.payload.data_ptr()))
        bad = torch.zeros((1,), dtype=torch.int64, device='cuda')
        kom.packing._launch_tile_crc(records, bad)
        assert int(bad.item()) == len(perturb)
        for c, e in exps:  # check mode writes nothing
            arena = c.arena_bytes()
            lo = G.GUARD
            assert (arena[:lo] == 0xA5).all() and (arena[lo + c.nbytes:] == 0xA5).all()
            assert np.array_equal(arena[lo:lo + c.nbytes].view(np.uint32), e)


def test_unusable_spans_count_as_bad_and_store_zero(kom, bundle):
    blob, dblob, table, recs, poff = bundle
    r = recs[1]  # u16, 4 tiles
    b = blob.tobytes()
    tab = list(struct.unpack('<4Q', b[r['toff']:r['toff'] + 32]))
    words = struct.unpack('<Q', b[56:64])[0]
    base = dblob.data_ptr()
    side, bw = base + r['side'], base + r['bw']
    g0 = S.tile_begin(blob)[1]
    # every payload pointer is the bundle's whole payload region (a wrong read would stay inside it)
    cases = {
        'backwards': ([tab[1], tab[0]], 0, words),                 # tile 0 runs from tab[1] back to tab[0]
        'past the window': ([tab[0], tab[1]], 0, tab[1] - 1),      # tile 0 ends 1 word past payload_words
        'before the window': ([tab[0], tab[1]], tab[0] + 1, words - tab[0] - 1),
        'too long': ([0, MAX_SPAN + 1], 0, words),
    }
    assert words > MAX_SPAN + 1
    for name, (entries, pfirst, pwords) in cases.items():
        tt = torch.tensor(entries, dtype=torch.int64, device='cuda')
        for mode in ('write', 'expect'):
            c = G.carve_arena((1,), torch.int32, 'cuda', 0x5A)
            G.fill(c, table[g0:g0 + 1].view(np.int32))  # in check mode: the right value, were the span usable
            bad = torch.zeros((1,), dtype=torch.int64, device='cuda')
            rec = (r['n'], 0, 0, side, bw, tt.data_ptr(), tt.data_ptr() + 8, base + poff + 4 * pfirst, pfirst, pwords,
                   c.payload.data_ptr() if mode == 'write' else None, None if mode == 'write' else c.payload.data_ptr())
            kom.packing._launch_tile_crc([rec], bad)
            assert int(bad.item()) == 1, (name, mode)
            got = int(c.payload.cpu().numpy().view(np.uint32)[0])
            assert got == (0 if mode == 'write' else int(table[g0])), (name, mode)
    # the same record, usable: the control
    tt = torch.tensor(tab[:2], dtype=torch.int64, device='cuda')
    out = torch.full((1,), -1, dtype=torch.int32, device='cuda')
    bad = torch.zeros((1,), dtype=torch.int64, device='cuda')
    kom.packing._launch_tile_crc([(r['n'], 0, 0, side, bw, tt.data_ptr(), tt.data_ptr() + 8, base + poff, 0, words,
                                   out.data_ptr(), None)], bad)
    assert int(bad.item()) == 0 and int(out.cpu().numpy().view(np.uint32)[0]) == int(table[g0])


def test_forty_records_take_two_launches(kom, bundle):
    blob, dblob, table, recs, poff = bundle
    begins = S.tile_begin(blob)
    ranges = [RANGES[q % len(RANGES)] for q in range(40)]
    buf, offs = _windows(bundle, ranges)
    wp = buf.data_ptr()
    out = torch.zeros((sum(t1 - t0 + 1 for _, t0, t1 in ranges),), dtype=torch.int32, device='cuda')
    records, at, want = [], 0, []
    for (a, t0, t1), (o_t, o_c, o_p, o_b, o_w, w0, pw) in zip(ranges, offs):
        records.append((recs[a]['n'], t0, t1, wp + o_p, wp + o_b, wp + o_t, wp + o_c, wp + o_w, w0, pw,
                        out.data_ptr() + 4 * at, None))
        at += t1 - t0 + 1
        want.append(table[begins[a] + t0:begins[a] + t1 + 1])
    kom.packing._launch_tile_crc(records, None)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), np.concatenate(want))


# ---------------------------------------------------------------------------------------------
# files
# ---------------------------------------------------------------------------------------------

def _volume(shape, dtype, seed=0):
    rng = np.random.default_rng(seed)
    g = np.indices(shape[1:4]).astype(np.float64)
    f = 60 * np.sin(g[0] / 5.0) + 40 * np.cos(g[1] / 3.0) + 30 * np.sin(g[2] / 4.0) + rng.normal(0, 2, shape[1:4])
    f = np.broadcast_to(f[None, ..., None], shape) + rng.normal(0, 1, shape)
    return (np.rint(f + 200).astype(np.int64) % (1 << (8 * np.dtype(dtype).itemsize))).astype(dtype)


def _split(raw):
    """``(metadata dict, metadata bytes, offset of the bundle)`` of file bytes."""
    mlen = struct.unpack('<4sHHQ', bytes(raw[:16]))[3]
    return json.loads(bytes(raw[16:16 + mlen])), mlen, 16 + mlen


@pytest.fixture(scope='module')
def crc_file(kom, tmp_path_factory):
    """The 43-tile file with a table, its bytes, the array, and what a test needs of its layout."""
    d = tmp_path_factory.mktemp('tilecrc')
    x = _volume((1, 40, 128, 128, 1), np.uint16, seed=4)
    path = d / 'g.kmp'
    info = kom.container.compress(str(path), x, kom.MeanPredictor(1, 3), levels=2, tile_crc=True)
    raw = path.read_bytes()
    assert info['bytes'] == len(raw)
    meta, mlen, base = _split(raw)
    bundle = raw[base:base + meta['bundle_bytes']]
    recs, poff = S.bundle_arrays(bundle)
    r = recs[1]  # level 0's first map [1, 20, 64, 64, 1]: planes [9, 11) are samples 36864 .. 45055, in tile 2 of 5
    assert r['nt'] == 5 and (9 * 64 * 64) // TILE == 2 == (11 * 64 * 64 - 1) // TILE
    tab = struct.unpack('<5Q', bundle[r['toff']:r['toff'] + 40])
    params = np.frombuffer(bundle, np.uint8, count=r['nb'], offset=r['side'])
    bw = np.frombuffer(bundle, np.uint8, count=r['nb'], offset=r['bw'])
    # a block of tile 2 inside the planes read, with at least one bit-plane: its first payload word is a plane word
    blk = next(k for k in range(9 * 64, 11 * 64) if params[k] >= 2)
    word = tab[2] + int(bw[512:blk].astype(np.int64).sum())
    return {'dir': d, 'path': str(path), 'raw': raw, 'x': x, 'meta': meta, 'base': base, 'bundle': bundle, 'poff': poff,
            'rec': r, 'tab': tab, 'blk': blk, 'word': word}


def _variant(f, name, at, flip=1, add=0):
    r = bytearray(f['raw'])
    r[at] = ((r[at] ^ flip) + add) & 0xff
    p = f['dir'] / name
    p.write_bytes(bytes(r))
    return str(p)


def test_trailer_is_the_spec_table_and_the_file_reads(kom, crc_file):
    f = crc_file
    meta, raw, base = f['meta'], f['raw'], f['base']
    n = meta['bundle_bytes']
    table = S.tile_crc_table(f['bundle'])
    assert meta['tile_crc'] == {'offset': n + (-n % 8), 'tiles': 43} and len(table) == 43
    off = base + meta['tile_crc']['offset']
    assert raw[base + n:off] == bytes(off - base - n) and len(raw) == off + 4 * 43
    assert np.array_equal(np.frombuffer(raw, '<u4', count=43, offset=off), table)
    assert kom.container.info(f['path'])['tile_crc'] == 43
    assert np.array_equal(kom.container.decompress(f['path']), f['x'])
    for kw in ({'planes': (18, 22)}, {'planes': (0, 40)}, {'planes': (39, 40)}, {}):
        got = kom.container.read_region(f['path'], **kw)
        z0, z1 = kw.get('planes', (0, 40))
        assert np.array_equal(got, f['x'][:, z0:z1])
        assert kom.container.last_timing['tile_crc'] is True
    assert np.array_equal(kom.container.read_region(f['path'], planes=(18, 22), tile_crc=False), f['x'][:, 18:22])
    assert kom.container.last_timing['tile_crc'] is False
    assert kom.container.check(f['path']) == {'ok': True, 'crc32': True, 'tile_crc': {'tiles': 43, 'bad': []}}


def test_batch_of_two(kom, tmp_path):
    x = _volume((2, 40, 128, 128, 1), np.uint16, seed=5)
    path = str(tmp_path / 'b2.kmp')
    kom.container.compress(path, x, kom.MeanPredictor(1, 3), levels=2, tile_crc=True)
    raw = open(path, 'rb').read()
    meta, mlen, base = _split(raw)
    table = S.tile_crc_table(raw[base:base + meta['bundle_bytes']])
    want = kom.container.plan_region(meta, batch=(0, 2))['tiles_total']
    assert meta['tile_crc']['tiles'] == want == len(table)
    assert np.array_equal(np.frombuffer(raw, '<u4', count=want, offset=base + meta['tile_crc']['offset']), table)
    assert np.array_equal(kom.container.read_region(path, batch=(1, 2)), x[1:2])
    assert kom.container.last_timing['tile_crc'] is True
    assert np.array_equal(kom.container.read_region(path, planes=(18, 22), batch=(0, 2)), x[:, 18:22])
    assert np.array_equal(kom.container.decompress(path), x)


def test_silent_corruption_is_caught(kom, crc_file):
    """A bit of a bit-plane word of a touched tile: every structural check passes and the samples are
    wrong -- without the per-tile CRC the read returns them; with it the read raises."""
    f = crc_file
    bad = _variant(f, 'plane.kmp', f['base'] + f['poff'] + 4 * f['word'] + 1, 0x10)
    got = kom.container.read_region(bad, planes=(18, 22), tile_crc=False)
    assert got.shape == f['x'][:, 18:22].shape and not np.array_equal(got, f['x'][:, 18:22])
    with pytest.raises(ValueError, match='tile CRC mismatch in 1 of the 15 tiles'):
        kom.container.read_region(bad, planes=(18, 22))
    with pytest.raises(ValueError, match=re.escape('(1, 2)')):
        kom.container.decompress(bad)
    assert kom.container.check(bad) == {'ok': False, 'crc32': False, 'tile_crc': {'tiles': 43, 'bad': [(1, 2)]}}


def test_params_byte_its_bw_still_admits(kom, crc_file):
    f = crc_file
    at = f['base'] + f['rec']['side'] + f['blk']
    assert f['raw'][at] >= 2
    bad = _variant(f, 'params.kmp', at, 0, -1)
    got = kom.container.read_region(bad, planes=(18, 22), tile_crc=False)
    assert not np.array_equal(got, f['x'][:, 18:22])
    with pytest.raises(ValueError, match='tile CRC mismatch'):
        kom.container.read_region(bad, planes=(18, 22))
    assert kom.container.check(bad)['tile_crc']['bad'] == [(1, 2)]


def test_untouched_damage_table_damage_and_truncation(kom, crc_file):
    f = crc_file
    want = f['x'][:, 18:22]
    far = _variant(f, 'far.kmp', f['base'] + f['poff'] + 4 * f['tab'][4] + 1, 0x10)  # tile 4: not touched
    assert np.array_equal(kom.container.read_region(far, planes=(18, 22)), want)
    with pytest.raises(ValueError):
        kom.container.read_region(far, planes=(18, 22), verify=True)
    assert kom.container.check(far)['tile_crc']['bad'] == [(1, 4)]
    # the table entry of tile 2 of array 1 (global index 1 + 2): a false alarm, never a silent pass
    entry = _variant(f, 'entry.kmp', f['base'] + f['meta']['tile_crc']['offset'] + 4 * 3 + 2, 0x04)
    with pytest.raises(ValueError, match='tile CRC mismatch'):
        kom.container.read_region(entry, planes=(18, 22))
    assert np.array_equal(kom.container.read_region(entry, planes=(18, 22), tile_crc=False), want)
    assert np.array_equal(kom.container.decompress(entry), f['x'])  # the bundle and its CRC are intact
    res = kom.container.check(entry)
    assert res['crc32'] is True and res['ok'] is False and res['tile_crc']['bad'] == [(1, 2)]
    # a trailer cut short
    (f['dir'] / 'trunc.kmp').write_bytes(f['raw'][:-4])
    with pytest.raises(ValueError, match='truncated per-tile CRC table'):
        kom.container.read_region(str(f['dir'] / 'trunc.kmp'), planes=(18, 22))
    res = kom.container.check(str(f['dir'] / 'trunc.kmp'))  # damage is reported, not raised
    assert res['ok'] is False and res['crc32'] is True


def _rewrite_meta(raw, meta):
    js = json.dumps(meta, separators=(',', ':')).encode()
    js += b' ' * (-len(js) % 8)
    return struct.pack('<4sHHQ', b'KMPF', 3, 0, len(js)) + js


def test_files_without_a_table(kom, crc_file, tmp_path):
    """The default keyword writes the parent's file byte for byte; a reader that ignores the key (the
    file with the key removed, trailer left in place) reads a file with a table exactly as before."""
    f = crc_file
    plain = str(tmp_path / 'plain.kmp')
    info = kom.container.compress(plain, f['x'], kom.MeanPredictor(1, 3), levels=2)
    raw = open(plain, 'rb').read()
    meta, mlen, base = _split(raw)
    assert 'tile_crc' not in meta and info['bytes'] == len(raw)
    body = raw[base:]
    assert len(body) == meta['bundle_bytes'] and body == f['bundle']  # the body IS the bundle, the same bundle
    stripped = {k: v for k, v in f['meta'].items() if k != 'tile_crc'}
    assert stripped == meta and _rewrite_meta(raw, stripped) + f['bundle'] == raw
    assert 'tile_crc' not in kom.container.info(plain)
    assert np.array_equal(kom.container.read_region(plain, planes=(18, 22)), f['x'][:, 18:22])
    assert kom.container.last_timing['tile_crc'] is False
    assert kom.container.check(plain) == {'ok': True, 'crc32': True, 'tile_crc': None}
    # the key ignored, the trailer still there
    keyless = str(tmp_path / 'keyless.kmp')
    open(keyless, 'wb').write(_rewrite_meta(raw, stripped) + f['raw'][f['base']:])
    assert np.array_equal(kom.container.decompress(keyless), f['x'])
    assert np.array_equal(kom.container.read_region(keyless, planes=(18, 22)), f['x'][:, 18:22])
    assert kom.container.last_timing['tile_crc'] is False
    lo, (maps, dims), m = kom.container.load(keyless)
    assert m['bundle_bytes'] == meta['bundle_bytes']
    # untouched damage in a file without a table is still not noticed
    r = bytearray(raw)
    r[base + f['poff'] + 4 * f['tab'][4] + 1] ^= 0x10
    open(str(tmp_path / 'far.kmp'), 'wb').write(bytes(r))
    assert np.array_equal(kom.container.read_region(str(tmp_path / 'far.kmp'), planes=(18, 22)), f['x'][:, 18:22])


def test_save_with_a_table_and_planes_refuses(kom, tmp_path):
    x = _volume((1, 40, 128, 128, 1), np.uint16, seed=6)
    pred = kom.MeanPredictor(0, 3)
    lo, enc = kom.volume.encode(pred, kom.volume.encode_values_uint16, x)
    path = str(tmp_path / 's.kmp')
    size = kom.container.save(path, lo, enc, predictor=pred, tile_crc=True)
    raw = open(path, 'rb').read()
    meta, mlen, base = _split(raw)
    assert size == len(raw) and meta['tile_crc']['tiles'] == len(S.tile_crc_table(raw[base:base + meta['bundle_bytes']]))
    assert np.array_equal(kom.container.read_region(path, planes=(18, 22)), x[:, 18:22])
    assert kom.container.last_timing['tile_crc'] is True
    for fn in (lambda: kom.container.compress(path, x, pred, method='planes', tile_crc=True),
               lambda: kom.container.save(path, lo, enc, predictor=pred, method='planes', tile_crc=True)):
        with pytest.raises(ValueError):
            fn()


def test_two_writes_are_identical(kom, crc_file, tmp_path):
    again = str(tmp_path / 'again.kmp')
    kom.container.compress(again, crc_file['x'], kom.MeanPredictor(1, 3), levels=2, tile_crc=True)
    assert open(again, 'rb').read() == crc_file['raw']
