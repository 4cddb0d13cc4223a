"""The Rice coder on inputs that reach every encode, decode and range path, and the decode path no
encoder reaches.

The bundles come from ``rice_spec``'s generators, whose census of control paths the CPU suite
asserts (``test_rice_spec.py``).  Encoder-reachable bundles are packed by the kernels and compared
byte for byte with ``oracle.rice.pack_bundle``.  Forced bundles (``rice_spec.pack_bundle_forced``:
valid by the format, a Rice parameter no encoder chooses, unary streams of 9 .. 2W + 2 words) exist
as bytes only; they and the others go through both decoders -- ``unpack_encoded`` and the ranged
launch with outputs carved from sentinel arenas -- twice each, bit-equal to the source arrays.
Look-back chains longer than the 64 tiles one round of the encoder's first wave covers are compared
byte for byte as well, and every check the decoders make on the side information is violated once.
"""

import numpy as np
import pytest
import torch

from oracle import rice as R
import guard_spec as G
import rice_spec as S

pytestmark = pytest.mark.gpu

TILE = S.TILE_SAMPLES
NP2T = {np.dtype(np.uint8): torch.uint8, np.dtype(np.uint16): torch.uint16, np.dtype(np.uint32): torch.uint32,
        np.dtype(np.int32): torch.int32, np.dtype(np.float32): torch.float32}


def _bits(a):
    return a.view(S.bits_dtype(a.dtype))


def _same(got, want):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(_bits(got), _bits(want))


def _encode(kom, arrays):
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]
    blob = kom.packing.pack_encoded(dev[0], (tuple(dev[1:]), ()))
    assert kom._lib.lib.kmp_last_launch() == b'rice_bundle_encode'
    return blob.cpu().numpy()


def _assert_bytes(got, want, what):
    assert got.size == want.size, (what, got.size, want.size)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f'{what}: {bad.size} bytes differ from the spec, first at {bad[:5].tolist()}'


def _decode_whole(kom, blob, arrays, what):
    """``unpack_encoded`` twice: the decode kernel served it, both results bit-equal to the source."""
    dblob = torch.from_numpy(blob).cuda()
    for run in range(2):
        lo, (maps, dims) = kom.packing.unpack_encoded(dblob)
        assert kom._lib.lib.kmp_last_launch() == b'rice_bundle_decode'
        got = (lo, *maps)
        assert len(got) == len(arrays) and dims == ()
        for q, (a, g) in enumerate(zip(arrays, got)):
            assert _same(g, a), f'{what}: array {q}, run {run}'


def _guards_intact(c):
    a = c.arena_bytes()
    lo = G.GUARD + c.shift
    return (a[:lo] == c.sentinel).all() and (a[lo + c.nbytes:] == c.sentinel).all()


def _body(c):
    lo = G.GUARD + c.shift
    return c.arena_bytes()[lo:lo + c.nbytes].copy()


def _launch(kom, blob, dblob, reqs, sentinel, base_at_first=False):
    """The ranged decode of ``reqs`` -- ``(array, first, end)`` -- from the resident bundle ``dblob``
    (whose bytes are ``blob``) into outputs carved from sentinel arenas.  A record's table window is
    its touched tiles' offsets closed by the next tile's or the record's end word; its payload window
    is the whole payload, or (``base_at_first``) starts at the record's first word.
    Returns ``(bad tiles, tiles launched, carved outputs, carved tables)``."""
    recs, poff, words = S.parse_bundle(blob)
    raw = blob.tobytes()
    base = dblob.data_ptr()
    outs, tabs, records = [], [], []
    for q, (i, f, e) in enumerate(reqs):
        code, n, nb, nt, side, toff, w_first, w_end = recs[i]
        dt = R.CODE_DTYPE[code]
        t0, t1 = f // TILE, (e - 1) // TILE
        tab = np.frombuffer(raw, np.uint64, count=nt, offset=toff)
        tl = np.concatenate([tab[t0:t1 + 1], [tab[t1 + 1] if t1 + 1 < nt else w_end]]).astype(np.uint64)
        c_t = G.fill(G.carve_arena((tl.size,), torch.int64, 'cuda', sentinel), tl.view(np.int64))
        c_o = G.carve_arena((e - f,), NP2T[dt], 'cuda', sentinel, shift=(q % 2) * 3 * dt.itemsize)
        tabs.append(c_t)
        outs.append(c_o)
        w0 = int(w_first) if base_at_first else 0
        bw_off = side + (nb + 7) // 8 * 8
        records.append((code, c_o.payload.data_ptr(), n, f, e, base + side + 256 * t0, base + bw_off + 256 * t0,
                        c_t.payload.data_ptr(), base + poff + 4 * w0, w0, words - w0))
    bad = torch.zeros((1,), dtype=torch.int64, device='cuda')
    tiles = kom.packing._launch_ranges(records, bad)
    assert kom._lib.lib.kmp_last_launch() == b'rice_bundle_decode_ranges'
    assert tiles == sum((e - 1) // TILE - f // TILE + 1 for _, f, e in reqs)
    return int(bad.item()), tiles, outs, tabs


def _decode_ranges(kom, blob, arrays, reqs, what):
    """``reqs`` through the ranged kernel on both sentinels: each range right, nothing outside it
    written, the table windows untouched, the two runs equal; then once through ``unpack_ranges``."""
    dblob = torch.from_numpy(blob).cuda()
    flat = [np.ascontiguousarray(a).reshape(-1) for a in arrays]
    runs = []
    for sentinel in G.SENTINELS:
        bad, _, outs, tabs = _launch(kom, blob, dblob, reqs, sentinel)
        assert bad == 0, what
        got = []
        for (i, f, e), c in zip(reqs, outs):
            assert _guards_intact(c), f'{what}: array {i} range [{f}, {e}) wrote outside its output'
            got.append(_body(c))
            assert np.array_equal(got[-1], flat[i][f:e].view(np.uint8)), f'{what}: array {i} range [{f}, {e})'
        assert all(_guards_intact(c) for c in tabs)
        runs.append(got)
    assert all(np.array_equal(x, y) for x, y in zip(*runs))
    for (i, f, e), g in zip(reqs, kom.packing.unpack_ranges(dblob, reqs)):
        assert _same(g, flat[i][f:e]), f'{what}: unpack_ranges array {i} range [{f}, {e})'


def _common_ranges(arrays):
    reqs = []
    for i, a in enumerate(arrays):
        n = a.size
        c = [(0, n), (0, 1), (n - 1, n), (9, 12), (3, 77), (64, 131), (509, 515), (512, 1024), (max(0, n - 70), n),
             (max(0, n - 7), n), (TILE - 5, TILE + 1), (TILE, TILE + 1)]
        reqs += [(i, f, e) for f, e in sorted(set(c)) if 0 <= f < e <= n]
    return reqs


def _forced_ranges(x, ks):
    """Ranges of the forced main array that begin and end inside a long block, inside a canonical
    block of a long step, and at the boundaries of a long step."""
    f = S.classify(x, ks)
    n = x.size
    nb = len(f['k'])
    step_long = np.zeros(-(-nb // 8), bool)
    np.logical_or.at(step_long, np.arange(nb) // 8, f['coded'] & f['long'])
    long_blocks = np.flatnonzero(f['coded'] & f['long'])
    inside = np.flatnonzero(f['coded'] & ~f['long'] & f['canonical'] & step_long[np.arange(nb) // 8])
    assert len(long_blocks) >= 24 and len(inside) >= 40
    c = []
    for b in long_blocks[[1, 7, 12, 17, 19, 23]]:
        c += [(64 * b + 5, 64 * b + 37), (64 * b + 63, 64 * b + 64)]
    for b in inside[[0, 11, 25, 39]]:
        c += [(64 * b + 3, 64 * b + 60), (64 * b + 17, 64 * b + 18)]
    for s in np.flatnonzero(step_long)[[0, 2, 5, 9]]:
        c += [(512 * s, 512 * s + 512), (512 * s + 505, 512 * s + 521), (512 * s, 512 * s + 1)]
    return [(0, int(a), int(b)) for a, b in c if 0 <= a < b <= n]


@pytest.mark.parametrize('i', range(S.NBUNDLES))
@pytest.mark.parametrize('W', S.WS)
def test_targeted_bundles(kom, W, i):
    """Bundle i of width W.  Encoder-reachable arrays: the kernels' bytes equal the oracle's.  They
    and the forced bundle of the same index: both decoders, twice each, bit-equal to the source."""
    arrays = S.reach_bundle(W, i)
    want = R.pack_bundle(arrays)
    _assert_bytes(_encode(kom, arrays), want, f'W={W} bundle {i} ({S.SIZE_KINDS[i]})')
    assert all(_same(b, a) for a, b in zip(arrays, R.unpack_bundle(want)[0]))
    _decode_whole(kom, want, arrays, f'W={W} bundle {i}')
    _decode_ranges(kom, want, arrays, _common_ranges(arrays), f'W={W} bundle {i}')
    farrays, ks = S.forced_bundle(W, i)
    fblob = S.pack_bundle_forced(farrays, ks)
    assert all(_same(b, a) for a, b in zip(farrays, R.unpack_bundle(fblob)[0]))
    _decode_whole(kom, fblob, farrays, f'W={W} forced bundle {i}')
    _decode_ranges(kom, fblob, farrays, _forced_ranges(farrays[0], ks[0]) + _common_ranges(farrays),
                   f'W={W} forced bundle {i}')


# ---------------------------------------------------------------------------------------------
# look-back chains past the 64 tiles of one round
# ---------------------------------------------------------------------------------------------

def _round_trip_exact(kom, arrays, what):
    want = R.pack_bundle(arrays)
    got = _encode(kom, arrays)
    _assert_bytes(got, want, what)  # header fields, side information, tile tables and payload
    _decode_whole(kom, got, arrays, what)


@pytest.mark.parametrize('ntile,dt', [(65, np.uint32), (66, np.uint32), (129, np.uint16), (200, np.uint8)])
def test_look_back_chain(kom, ntile, dt):
    """One launch of 65, 129 and 200 tiles, each mostly zero blocks with 1 .. 7 coded ones: a tile's
    start is the sum of up to 199 aggregates that differ from tile to tile.  The last of 65 tiles
    reads all 64 lanes' worth of predecessors in its first round; 66 is the first count at which a
    second round (``base -= 64``) can be needed.  Whether a tile takes that round is a matter of
    scheduling -- only when its 64 nearest predecessors have all published an aggregate and no prefix
    yet when it reads them -- and nothing here can observe it: these cases pin the bytes whichever
    way the chain was walked, they do not guarantee that the second round ran."""
    _round_trip_exact(kom, [S.sparse_tiles(ntile, dt, 7)], f'{ntile} tiles of {np.dtype(dt).name}')


def test_look_back_across_launches(kom):
    """uint8 x 70 tiles, uint16 x 70 tiles, uint8 x 3 tiles: three launches on one chain of 143 tiles,
    the second and third starting at ``tile_begin`` = 70 and 140."""
    arrays = [S.sparse_tiles(70, np.uint8, 1), S.sparse_tiles(70, np.uint16, 2), S.sparse_tiles(3, np.uint8, 3)]
    _round_trip_exact(kom, arrays, 'three launches')


# ---------------------------------------------------------------------------------------------
# corruption: every check of the decoders violated once
# ---------------------------------------------------------------------------------------------

CORRUPTIONS = ('param 0 with bw != 0', 'k >= W', 'bw < 2k + 2', 'bw > 2W + 2', 'tile offset past payload_words',
               'tile offset breaks start + agg == end', 'record first word', 'record end word')


@pytest.fixture(scope='module')
def victims():
    """Per width: two arrays of one dtype -- three tiles (the targeted blocks in tile 0, Laplacian
    residuals after them) and less than one tile -- their bundle, and the ranges asked of it."""
    out = {}
    for W in S.WS:
        dt = S.DTYPES[W][0]
        rng = np.random.default_rng(W)
        head = S.reach_bundle(W, 0)[0].view(dt)
        a0 = np.concatenate([head, S.to_samples(S.filler_blocks(3 * 256, rng, 2.0), dt, 3 * TILE - 100 - head.size)])
        a1 = S.reach_bundle(W, 1)[0].view(dt)
        n0, n1 = a0.size, a1.size
        reqs = [(0, 100, 900), (0, TILE - 300, TILE + 200), (0, TILE + 50, 2 * TILE + 50), (0, 2 * TILE + 10, n0 - 5),
                (1, 10, n1 - 3), (0, 0, n0)]
        out[W] = ([a0, a1], R.pack_bundle([a0, a1]), reqs)
    return out


def _move_words(g, bw_off, f, W, victim, value, tile):
    """Sets ``bw[victim] = value`` and moves the opposite difference onto another coded block of the
    same tile that stays within [2k + 2, 2W + 2]: the tile's word sum still equals ``end - start``,
    so the victim's own range check is the only one the tile fails."""
    delta = int(value) - int(g[bw_off + victim])
    room = f['coded'] & tile & (np.arange(len(tile)) != victim) & \
        (f['bw'] - delta >= 2 * f['k'] + 2) & (f['bw'] - delta <= 2 * W + 2)
    other = np.flatnonzero(room)[0]
    g[bw_off + victim] = value
    g[bw_off + other] = f['bw'][other] - delta
    k, w = f['k'][other], int(g[bw_off + other])
    assert 2 * k + 2 <= w <= 2 * W + 2
    n = int(tile.sum())
    assert g[bw_off:bw_off + n].astype(np.int64).sum() == f['bw'][:n].sum()


def _corrupt(blob, arrays, W, what):
    """``(corrupt copy, {(array, tile)} that hold the corruption, base_at_first)``.  The four
    side-information cases violate the per-block check alone: ``k >= W`` changes a param byte only,
    and the three that change a ``bw`` byte keep the tile's word sum (``_move_words``), so without the
    per-block check the tile would pass.  A tile offset or a record's end word can only be wrong
    through ``start + agg == end`` or the payload extent: those cases are coupled with the sum check
    by nature, and a wrong offset makes the tile before it and the tile at it bad."""
    recs, poff, words = S.parse_bundle(blob)
    code, n, nb, nt, side, toff, w_first, w_end = recs[0]
    bw_off = side + (nb + 7) // 8 * 8
    f = S.classify(arrays[0])
    tile0 = np.arange(nb) < 256
    g = blob.copy()
    bad = {(0, 0)}
    base_at_first = False
    if what == 'param 0 with bw != 0':
        _move_words(g, bw_off, f, W, np.flatnonzero(~f['coded'] & tile0)[0], 2, tile0)
    elif what == 'k >= W':
        g[side + np.flatnonzero((f['bw'] == 2 * W + 2) & tile0)[0]] = W + 1
    elif what == 'bw < 2k + 2':
        b = np.flatnonzero(f['coded'] & (f['k'] >= 2) & tile0)[0]
        _move_words(g, bw_off, f, W, b, 2 * f['k'][b] + 1, tile0)
    elif what == 'bw > 2W + 2':
        _move_words(g, bw_off, f, W, np.flatnonzero((f['bw'] == 2 * W + 2) & tile0)[0], 2 * W + 3, tile0)
    elif what.startswith('tile offset'):
        tab = g[toff:toff + 8 * nt].view(np.uint64)
        tab[1] = words + 5 if 'past' in what else tab[1] + 1
        bad = {(0, 0), (0, 1)}
    elif what == 'record first word':
        g[80 + 128 + 112:80 + 128 + 120].view(np.uint64)[0] += 1
        bad, base_at_first = {(1, 0)}, True
    else:
        g[80 + 120:80 + 128].view(np.uint64)[0] -= 1
        bad = {(0, nt - 1)}
    assert not np.array_equal(g, blob)
    return g, bad, base_at_first


@pytest.mark.parametrize('what', CORRUPTIONS)
@pytest.mark.parametrize('W', S.WS)
def test_corruption(kom, victims, W, what):
    """One corruption (``_corrupt`` says which check each violates): the whole decode raises; the
    ranged launch counts exactly the touched tiles that hold it, writes zeros for them, decodes every
    other tile of the call, and leaves the guards alone."""
    arrays, blob, reqs = victims[W]
    g, bad_tiles, base_at_first = _corrupt(blob, arrays, W, what)
    with pytest.raises(ValueError):
        kom.packing.unpack_encoded(g)
    dblob = torch.from_numpy(g).cuda()
    for sentinel in G.SENTINELS:
        bad, _, outs, tabs = _launch(kom, g, dblob, reqs, sentinel, base_at_first)
        want_bad = sum((i, t) in bad_tiles for i, f, e in reqs for t in range(f // TILE, (e - 1) // TILE + 1))
        assert want_bad >= 1 and bad == want_bad, (what, bad, want_bad)
        for (i, f, e), c in zip(reqs, outs):
            want = arrays[i][f:e].copy()
            for t in range(f // TILE, (e - 1) // TILE + 1):
                if (i, t) in bad_tiles:
                    want[max(f, t * TILE) - f:min(e, (t + 1) * TILE) - f] = 0
            assert _guards_intact(c), f'{what}: array {i} range [{f}, {e}) wrote outside its output'
            assert np.array_equal(_body(c), want.view(np.uint8)), f'{what}: array {i} range [{f}, {e})'
        assert all(_guards_intact(c) for c in tabs)


@pytest.mark.parametrize('W', S.WS)
def test_random_payload_under_intact_side_information(kom, victims, W):
    """Tile 1 of the first array holds random words under its own side information.  No value is
    asserted for that tile (content is the CRC layer's job): every read of the stream is bounded by
    the block's word count, so the call returns, writes only inside its outputs, and two runs agree;
    the ranges that do not touch the tile are right."""
    arrays, blob, reqs = victims[W]
    recs, poff, words = S.parse_bundle(blob)
    code, n, nb, nt, side, toff, w_first, w_end = recs[0]
    tab = np.frombuffer(blob.tobytes(), np.uint64, count=nt, offset=toff)
    g = blob.copy()
    lo, hi = int(tab[1]), int(tab[2])
    g[poff + 4 * lo:poff + 4 * hi] = np.random.default_rng(W).integers(0, 256, 4 * (hi - lo), dtype=np.uint8)
    dblob = torch.from_numpy(g).cuda()
    runs = []
    for sentinel in G.SENTINELS:
        bad, _, outs, tabs = _launch(kom, g, dblob, reqs, sentinel)
        assert bad == 0  # the side information is intact
        assert all(_guards_intact(c) for c in outs + tabs)
        runs.append([_body(c) for c in outs])
        for (i, f, e), got in zip(reqs, runs[-1]):
            if i != 0 or e <= TILE or f >= 2 * TILE:
                assert np.array_equal(got, arrays[i][f:e].view(np.uint8)), f'array {i} range [{f}, {e})'
    assert all(np.array_equal(x, y) for x, y in zip(*runs))
