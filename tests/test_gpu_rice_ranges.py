"""Rice decode of sample ranges (kmp_rice_bundle_decode_ranges, packing.unpack_ranges).

A range ``[first, end)`` of an array of a v2 bundle must come out bit-equal to the slice of the
SOURCE array (the bundles are byte-pinned to oracle/rice.py elsewhere; one case here packs with
the oracle directly), whatever tiles it touches, with nothing written outside its output, from a
resident bundle and from separate windows that hold exactly the touched tiles' side information,
table entries and payload words between sentinel bytes -- the situation of a partial file read.

Arrays: every n at which the tile / block / lane structure changes (one sample; one short block;
exactly one block; one block and a sample; exactly one tile; one tile and a sample; a short last
block in a third tile; three tiles and 17 samples) times four residual patterns (all-zero blocks,
Laplacian sigma ~ 2, full-range random, one huge value among zeros), per sample width and dtype."""

import struct

import numpy as np
import pytest
import torch

from oracle import rice as R
import guard_spec as G

pytestmark = pytest.mark.gpu

TILE = 16384
NS = (1, 63, 64, 65, 16384, 16385, 40000, 3 * 16384 + 17)
DTYPES = {'u8': np.uint8, 'u16': np.uint16, 'u32': np.uint32, 'i32': np.int32, 'f32': np.float32}
NP2T = {np.uint8: torch.uint8, np.uint16: torch.uint16, np.uint32: torch.uint32, np.int32: torch.int32,
        np.float32: torch.float32}
KINDS = ('zeros', 'laplace', 'random', 'lopsided')


def _bits(dt):
    return np.dtype({np.float32: np.uint32, np.int32: np.uint32}.get(dt, dt))


def _array(kind, n, dt, rng):
    """``n`` samples of ``dt`` whose bit patterns are W-bit residuals of ``kind``."""
    u = _bits(dt)
    W = 8 * u.itemsize
    if kind == 'zeros':
        v = np.zeros(n, np.int64)
    elif kind == 'laplace':
        v = np.rint(rng.laplace(0.0, 2.0 / np.sqrt(2.0), n)).astype(np.int64)
    elif kind == 'random':
        v = rng.integers(0, 1 << W, n, dtype=np.int64)
    else:  # one huge value per block of 64 among zeros: a long unary part
        v = np.zeros(n, np.int64)
        for b0 in range(0, n, 64):
            mag = int(rng.choice([40, 200, 1000, 30000, (1 << (W - 1)) - 1]))
            v[b0 + int(rng.integers(0, min(64, n - b0)))] = min(mag, (1 << (W - 1)) - 1) * int(rng.choice([-1, 1]))
    return (v & ((1 << W) - 1)).astype(u).view(dt)


def _structured(n):
    """The ranges of the issue's list that exist in an array of n samples."""
    c = [(0, n), (0, 1), (n - 1, n), (n // 2, n // 2 + 1),
         (9, 12), (16, 19),                                    # within one lane
         (3, 77), (8, 130), (5, 64), (64, 131), (65, 200),     # off / on multiples of 8 and 64
         (TILE - 1, TILE + 1), (TILE - 5, TILE + 1), (TILE, TILE + 1), (TILE - 1, TILE),  # across a tile boundary
         (TILE + 3, 2 * TILE + 9), (100, 2 * TILE), (TILE, 2 * TILE), (2 * TILE - 64, 2 * TILE + 64),
         (max(0, n - 70), n), (max(0, n - 7), n), (max(0, n - TILE - 3), n)]  # ending at n (short last block)
    return sorted({(f, e) for f, e in c if 0 <= f < e <= n})


def _parse(blob):
    """Per array ``(code, n, nb, ntile, side, toff, first word, end word)`` plus ``(payload_off,
    words)`` of a v2 bundle, parsed here from the bytes (oracle/rice.py pack_bundle's layout)."""
    b = blob.tobytes()
    count = struct.unpack('<H', b[6:8])[0]
    poff, words = struct.unpack('<2Q', b[48:64])
    recs = []
    for i in range(count):
        r = b[80 + 128 * i:80 + 128 * (i + 1)]
        code = struct.unpack('<I', r[:4])[0]
        n, nb, nt, side, toff, first, end = struct.unpack('<5q2Q', r[72:128])
        recs.append((code, n, nb, nt, side, toff, first, end))
    return recs, poff, words


@pytest.fixture(scope='module')
def bundles(kom):
    """Per dtype: ``(source arrays, bundle bytes (numpy), resident bundle (device))`` of all NS x
    KINDS arrays, packed once by pack_encoded."""
    out = {}
    for seed, (name, dt) in enumerate(DTYPES.items()):
        rng = np.random.default_rng(100 + seed)
        arrs = [_array(k, n, dt, rng) for n in NS for k in KINDS]
        blob = kom.packing.pack_encoded(arrs[0], (tuple(arrs[1:]), ()))
        out[name] = (arrs, blob, torch.from_numpy(blob).cuda())
    return out


def _same(got, want):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    return got.dtype == want.dtype and got.shape == want.shape and \
        np.array_equal(got.view(_bits(want.dtype.type)), want.view(_bits(want.dtype.type)))


@pytest.mark.parametrize('name', list(DTYPES))
def test_structured_ranges(kom, bundles, name):
    arrs, blob, dblob = bundles[name]
    reqs = [(i, f, e) for i, a in enumerate(arrs) for f, e in _structured(a.size)]
    got = kom.packing.unpack_ranges(dblob, reqs)
    assert kom._lib.lib.kmp_last_launch() == b'rice_bundle_decode_ranges'
    assert len(got) == len(reqs)
    for (i, f, e), g in zip(reqs, got):
        assert _same(g, arrs[i][f:e]), f'{name}: array {i} (n = {arrs[i].size}) range [{f}, {e})'


@pytest.mark.parametrize('name', list(DTYPES))
def test_random_ranges(kom, bundles, name):
    arrs, blob, dblob = bundles[name]
    rng = np.random.default_rng(2024)
    reqs = []
    for _ in range(200):
        i = int(rng.integers(0, len(arrs)))
        n = arrs[i].size
        f = int(rng.integers(0, n))
        e = min(n, f + 1 + int(rng.integers(0, 100))) if rng.random() < 0.5 else int(rng.integers(f + 1, n + 1))
        reqs.append((i, f, e))
    got = kom.packing.unpack_ranges(blob, reqs)  # numpy in -> numpy out
    for (i, f, e), g in zip(reqs, got):
        assert isinstance(g, np.ndarray) and _same(g, arrs[i][f:e]), f'{name}: array {i} range [{f}, {e})'


def test_forty_records_in_one_call(kom, bundles):
    arrs, blob, dblob = bundles['u16']
    i = len(arrs) - 3  # 3 tiles + 17 samples, Laplacian
    reqs = [(i, 1000 * q + q, 1000 * q + q + 700 + 13 * q) for q in range(40)]
    got = kom.packing.unpack_ranges(dblob, reqs)
    for (_, f, e), g in zip(reqs, got):
        assert _same(g, arrs[i][f:e])


def test_mixed_dtypes_and_oracle_bytes(kom):
    """Three arrays of mixed dtype (a record's first word is not 0, launches split by dtype), once
    packed by pack_encoded and once by the oracle's pack_bundle: the same ranges from both."""
    rng = np.random.default_rng(5)
    arrs = [_array('laplace', 40000, np.uint16, rng), _array('random', 3 * TILE + 17, np.uint8, rng),
            _array('lopsided', 16385, np.int32, rng), _array('laplace', 20000, np.uint16, rng)]
    reqs = [(i, f, e) for i, a in enumerate(arrs) for f, e in _structured(a.size)]
    for blob in (kom.packing.pack_encoded(arrs[0], (tuple(arrs[1:]), ())), R.pack_bundle(arrs)):
        got = kom.packing.unpack_ranges(blob, reqs)
        for (i, f, e), g in zip(reqs, got):
            assert _same(g, arrs[i][f:e]), f'array {i} range [{f}, {e})'


def test_requests_are_checked(kom, bundles):
    arrs, blob, dblob = bundles['u8']
    for bad in [(len(arrs), 0, 1), (-1, 0, 1), (0, 0, 0), (0, 1, 0), (0, 0, arrs[0].size + 1), (4, -1, 3)]:
        with pytest.raises(ValueError):
            kom.packing.unpack_ranges(dblob, [bad])
    with pytest.raises(ValueError):
        kom.packing.unpack_ranges(kom.packing.pack_encoded(arrs[0], ((arrs[1],), ()), 'planes'), [(0, 0, 1)])
    assert kom.packing.unpack_ranges(dblob, []) == []


# ---------------------------------------------------------------------------------------------
# the launch itself: outputs carved from sentinel arenas; windows between sentinels
# ---------------------------------------------------------------------------------------------

def _records(kom, blob, dblob, reqs, outs, windowed, sentinel, keep):
    """Launch records for ``reqs`` writing into the device tensors ``outs``.  ``windowed``: the side
    information, the table entries and the payload words of the touched tiles ONLY, each copied
    into a buffer of its own between guard bytes; else pointers into the resident bundle (the
    table window, which needs its closing entry, is built from the host values either way)."""
    recs, poff, words = _parse(blob)
    out = []
    for (i, f, e), o in zip(reqs, outs):
        code, n, nb, nt, side, toff, w_first, w_end = recs[i]
        t0, t1 = f // TILE, (e - 1) // TILE
        tab = np.frombuffer(blob.tobytes(), np.uint64, count=nt, offset=toff)
        tl = np.concatenate([tab[t0:t1 + 1], [tab[t1 + 1] if t1 + 1 < nt else w_end]]).astype(np.uint64)
        c_t = G.carve_arena((tl.size,), torch.int64, 'cuda', sentinel)
        G.fill(c_t, tl.view(np.int64))
        keep.append(c_t)
        nside = min(nb, 256 * (t1 + 1)) - 256 * t0
        bw_off = side + (nb + 7) // 8 * 8
        if windowed:
            c_p = G.fill(G.carve_arena((nside,), torch.uint8, 'cuda', sentinel, shift=1),
                         blob[side + 256 * t0:side + 256 * t0 + nside])
            c_b = G.fill(G.carve_arena((nside,), torch.uint8, 'cuda', sentinel, shift=3),
                         blob[bw_off + 256 * t0:bw_off + 256 * t0 + nside])
            pw = int(tl[-1] - tl[0])
            if pw:
                c_w = G.fill(G.carve_arena((pw,), torch.int32, 'cuda', sentinel, shift=4),
                             blob[poff + 4 * int(tl[0]):poff + 4 * int(tl[-1])].view(np.int32))
            else:  # all-zero tiles have no payload: zero readable words at a sentinel word
                c_w = G.carve_arena((1,), torch.int32, 'cuda', sentinel, shift=4)
            keep += [c_p, c_b, c_w]
            pp, bp, wp, w0 = c_p.payload.data_ptr(), c_b.payload.data_ptr(), c_w.payload.data_ptr(), int(tl[0])
        else:
            base = dblob.data_ptr()
            pp, bp, wp, w0, pw = base + side + 256 * t0, base + bw_off + 256 * t0, base + poff, 0, words
        out.append((code, o.data_ptr(), n, f, e, pp, bp, c_t.payload.data_ptr(), wp, w0, pw))
    return out


@pytest.mark.parametrize('windowed', [False, True], ids=['resident', 'windows'])
@pytest.mark.parametrize('name', list(DTYPES))
def test_guarded_outputs(kom, bundles, name, windowed):
    """Outputs carved from sentinel arenas (shifted by 0 and by an odd element count): the range is
    right, no byte outside ``[0, end - first)`` is written, two runs on two sentinels agree, and the
    ranged kernel served the call -- from the resident bundle and from exact windows."""
    arrs, blob, dblob = bundles[name]
    dt = DTYPES[name]
    item = np.dtype(dt).itemsize
    picks = [i for i, a in enumerate(arrs) if a.size in (65, 16385, 3 * TILE + 17)]
    reqs = [(i, f, e) for i in picks for f, e in _structured(arrs[i].size)]
    runs = []
    for sentinel in G.SENTINELS:
        keep = []
        carved = [G.carve_arena((e - f,), NP2T[dt], 'cuda', sentinel, shift=(q % 2) * 3 * item)
                  for q, (i, f, e) in enumerate(reqs)]
        records = _records(kom, blob, dblob, reqs, [c.payload for c in carved], windowed, sentinel, keep)
        bad = torch.zeros((1,), dtype=torch.int64, device='cuda')
        tiles = kom.packing._launch_ranges(records, bad)
        assert kom._lib.lib.kmp_last_launch() == b'rice_bundle_decode_ranges'
        assert int(bad.item()) == 0
        assert tiles == sum((e - 1) // TILE - f // TILE + 1 for _, f, e in reqs)
        got = []
        for (i, f, e), c in zip(reqs, carved):
            a = c.arena_bytes()
            lo = G.GUARD + c.shift
            body = a[lo:lo + c.nbytes]
            assert (a[:lo] == sentinel).all() and (a[lo + c.nbytes:] == sentinel).all(), \
                f'{name}: array {i} range [{f}, {e}) wrote outside its output'
            assert np.array_equal(body, arrs[i][f:e].view(np.uint8)), f'{name}: array {i} range [{f}, {e})'
            got.append(body.copy())
        for c in keep:  # the inputs and their guards are untouched
            a = c.arena_bytes()
            lo = G.GUARD + c.shift
            assert (a[:lo] == sentinel).all() and (a[lo + c.nbytes:] == sentinel).all()
        runs.append(got)
    assert all(np.array_equal(x, y) for x, y in zip(*runs))


def test_unselected_parts_are_not_read(kom, bundles):
    """Garbage over the side information and the payload of every tile a range does not touch
    changes nothing (the table and the header stay)."""
    arrs, blob, dblob = bundles['u16']
    i = len(arrs) - 3  # 3 tiles + 17 samples, Laplacian: tiles 0 .. 3
    recs, poff, words = _parse(blob)
    code, n, nb, nt, side, toff, w_first, w_end = recs[i]
    tab = np.frombuffer(blob.tobytes(), np.uint64, count=nt, offset=toff)
    f, e = TILE + 100, 2 * TILE - 50  # inside tile 1
    g = blob.copy()
    rng = np.random.default_rng(1)
    bw_off = side + (nb + 7) // 8 * 8
    for lo, hi in ((0, 256), (512, nb)):  # blocks of tiles 0, 2 and 3
        g[side + lo:side + hi] = rng.integers(0, 256, hi - lo, dtype=np.uint8)
        g[bw_off + lo:bw_off + hi] = rng.integers(0, 256, hi - lo, dtype=np.uint8)
    for lo, hi in ((int(w_first), int(tab[1])), (int(tab[2]), int(w_end))):
        g[poff + 4 * lo:poff + 4 * hi] = rng.integers(0, 256, 4 * (hi - lo), dtype=np.uint8)
    assert not np.array_equal(g, blob)
    (got,) = kom.packing.unpack_ranges(g, [(i, f, e)])
    assert _same(got, arrs[i][f:e])


def test_corruption_in_touched_and_untouched_tiles(kom, bundles):
    arrs, blob, dblob = bundles['u16']
    i = len(arrs) - 3
    recs, poff, words = _parse(blob)
    code, n, nb, nt, side, toff, w_first, w_end = recs[i]
    bw_off = side + (nb + 7) // 8 * 8
    f, e = TILE + 100, 2 * TILE - 50  # tile 1 = blocks 256 .. 511
    hit = blob.copy()
    hit[bw_off + 300] ^= 1  # a block of the touched tile, outside the range's own blocks or not
    with pytest.raises(ValueError):
        kom.packing.unpack_ranges(hit, [(i, f, e)])
    miss = blob.copy()
    miss[bw_off + 700] ^= 1  # tile 2
    (got,) = kom.packing.unpack_ranges(miss, [(i, f, e)])
    assert _same(got, arrs[i][f:e])
    with pytest.raises(ValueError):  # the whole-bundle decode does notice it
        kom.packing.unpack_encoded(miss)
