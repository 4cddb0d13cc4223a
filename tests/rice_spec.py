"""A path model of the Rice coder (kmp_rice.hip; spec oracle/rice.py), in plain numpy.

Three things the Rice tests share:

* ``pack_forced`` / ``pack_bundle_forced``: the specification's packer with the Rice parameter
  given per block.  The format fixes no rule for k: ``oracle.rice.unpack``, both decode kernels and
  the side-information check take any k < W with 2k + 2 <= bw <= 2W + 2.  The project's encoder
  always writes k* (the smallest k minimising the block's words), for which the unary part never
  exceeds 7 words (``unary_words_bound``); a forced k reaches the decoders' paths for longer
  streams, which no bundle of the encoder's takes.
* ``census``: which control paths of the kernels an array reaches, by the kernels' own conditions
  restated here -- per wave step of 8 blocks (encoder ``lo``; decoder ``lo8``, ``short_stream``),
  per block (k*, ties, zero blocks, the 32-bit sum cap) and per lane of 8 samples (the encoder's one
  mask against per-bit ORs; the decoder's 32-bit window, 64-bit window and word walk).
* seeded generators that build blocks from a target (a k*, a tie, a lane length, a stream
  length) and ``reach_bundle`` / ``forced_bundle``, the eight bundles per sample width that the CPU
  suite takes the census of (test_rice_spec.py) and the GPU suite runs (test_gpu_rice_paths.py).

Blocks are built in the zigzag domain (``z``, uint64[64]) and turned into samples at the end.
"""

from collections import Counter
import struct

import numpy as np

from oracle import rice as R
from oracle.packing import BLOCK, _blocks, sample_bits, unzigzag, zigzag

STEP = 8                 # blocks per wave step
STEP_SAMPLES = STEP * BLOCK
TILE_SAMPLES = R.TILE_BLOCKS * BLOCK
CAP = 1 << 20            # kSumCap
WS = (8, 16, 32)
DTYPES = {8: (np.uint8,), 16: (np.uint16,), 32: (np.int32, np.uint32, np.float32)}
NBUNDLES = 8             # bundles per sample width and kind; bundle i ends on size kind i
SIZE_KINDS = ('lane', 'lane + 1', 'block', 'block + 1', 'step', 'step + 1', 'tile', 'tile + 1')


def bits_dtype(dt):
    return np.dtype(f'u{np.dtype(dt).itemsize}')


def tables(zb, W):
    """``(S, words)``, int64 ``[nb, W + 1]``: S_k and words(k) of every block, k = 0 .. W."""
    S = np.stack([(zb >> np.uint64(k)).sum(axis=1) for k in range(W + 1)], axis=1).astype(np.int64)
    return S, 2 * np.arange(W + 1)[None, :] + (64 + S + 31) // 32


def unary_words_bound(W, k):
    """The most unary words the encoder's k* = k can have.  With u = uw(k) and S_{k+1} <= S_k / 2,
    uw(k + 1) <= 1 + ceil(u / 2), so words(k + 1) <= 2k + 3 + ceil(u / 2) < 2k + u = words(k) for
    u >= 8: such a k < W - 1 is never the minimum.  At k = W - 1, S_k <= 64 and uw <= 4."""
    return 7 if k < W - 1 else 4


# ---------------------------------------------------------------------------------------------
# the packer with k given per block
# ---------------------------------------------------------------------------------------------

def plan_forced(x, ks=None):
    """``(W, zb, params, bw, S, words, kstar, zero)`` of the flat array ``x`` with the Rice parameter
    of block b forced to ``ks[b]``: ``None`` = k*, ``-1`` = param 0 (the block must be all zero)."""
    x = np.ascontiguousarray(np.asarray(x).reshape(-1))
    W = sample_bits(x.dtype)
    zb = _blocks(zigzag(x, W))
    nb = zb.shape[0]
    S, words = tables(zb, W)
    zero = (zb == 0).all(axis=1)
    kstar = np.argmin(words, axis=1) if nb else np.zeros(0, np.int64)
    params = np.where(zero, 0, kstar + 1).astype(np.int64)
    bw = np.where(zero, 0, words[np.arange(nb), kstar]).astype(np.int64)
    if ks is not None:
        assert len(ks) == nb, (len(ks), nb)
        for b, kf in enumerate(ks):
            if kf is None:
                continue
            if kf == -1:
                assert zero[b], f'block {b}: param 0 on a block that is not all zero'
                params[b] = bw[b] = 0
            else:
                assert 0 <= kf < W, (b, kf)
                assert words[b, kf] <= 2 * W + 2, f'block {b}: k = {kf} needs {words[b, kf]} words'
                params[b], bw[b] = kf + 1, words[b, kf]
    return W, zb, params.astype(np.uint8), bw.astype(np.uint8), S, words, kstar, zero


def pack_forced(x, ks=None):
    """``(params, bw, payload)`` as ``oracle.rice.pack``, the parameter of block b forced to ``ks[b]``."""
    W, zb, params, bw, *_ = plan_forced(x, ks)
    nb = zb.shape[0]
    off = np.zeros(nb + 1, np.int64)
    np.cumsum(bw.astype(np.int64), out=off[1:])
    payload = np.zeros(int(off[-1]), np.uint32)
    lanes = np.arange(BLOCK, dtype=np.uint64)
    for blk in np.nonzero(params)[0]:
        k = int(params[blk]) - 1
        z = zb[blk]
        o = int(off[blk])
        for b in range(k):
            plane = int(np.bitwise_or.reduce(((z >> np.uint64(b)) & np.uint64(1)) << lanes))
            payload[o + 2 * b] = plane & 0xffffffff
            payload[o + 2 * b + 1] = plane >> 32
        pos = np.cumsum((z >> np.uint64(k)).astype(np.int64) + 1) - 1
        np.bitwise_or.at(payload, o + 2 * k + (pos >> 5), (np.uint32(1) << (pos & 31).astype(np.uint32)))
    return params, bw, payload


def pack_bundle_forced(arrays, ks_per_array, dims=()):
    """``oracle.rice.pack_bundle``'s bytes with the parameters of array a forced to ``ks_per_array[a]``
    (``None``: k* everywhere)."""
    arrays = [np.ascontiguousarray(a) for a in arrays]
    head, offs, poff = R.bundle_layout([a.size for a in arrays])
    words, recs, parts = 0, [], []
    for a, ks in zip(arrays, ks_per_array):
        params, bw, payload = pack_forced(a.reshape(-1), ks)
        nb = len(params)
        boff = np.zeros(nb + 1, np.int64)
        np.cumsum(bw.astype(np.int64), out=boff[1:])
        tiles = (words + boff[:-1][::R.TILE_BLOCKS]).astype(np.uint64) if nb else np.zeros(0, np.uint64)
        first, end = (words, words + int(boff[-1])) if nb else (0, 0)
        recs.append((params, bw, tiles, first, end))
        parts.append(payload)
        words += int(boff[-1]) if nb else 0
    total = poff + R._pad8(4 * words)
    out = np.zeros(total, np.uint8)
    hdr = struct.pack('<4sHHII', b'KMPB', 2, len(arrays), len(dims), 0)
    hdr += struct.pack('<8i', *(list(int(d) for d in dims) + [0] * (8 - len(dims))))
    hdr += struct.pack('<4Q', poff, words, total, 0)
    for a, (side, toff), (params, bw, tiles, first, end) in zip(arrays, offs, recs):
        nb = len(params)
        hdr += struct.pack('<II8q', R.DTYPE_CODE[a.dtype], a.ndim, *(list(a.shape) + [0] * (8 - a.ndim)))
        hdr += struct.pack('<5q2Q', a.size, nb, len(tiles), side, toff, first, end)
        out[side:side + nb] = params
        out[side + R._pad8(nb):side + R._pad8(nb) + nb] = bw
        out[toff:toff + 8 * len(tiles)] = tiles.view(np.uint8)
    out[:head] = np.frombuffer(hdr, np.uint8)
    if words:
        out[poff:poff + 4 * words] = np.concatenate(parts).astype(np.uint32).view(np.uint8)
    return out


def parse_bundle(blob):
    """``([(code, n, nb, ntile, side_off, toff_off, first word, end word)], payload_off, words)``."""
    b = np.asarray(blob, np.uint8).tobytes()
    count = struct.unpack('<H', b[6:8])[0]
    poff, words = struct.unpack('<2Q', b[48:64])
    recs = []
    for i in range(count):
        r = b[80 + 128 * i:80 + 128 * (i + 1)]
        recs.append((struct.unpack('<I', r[:4])[0], *struct.unpack('<5q2Q', r[72:128])))
    return recs, poff, words


# ---------------------------------------------------------------------------------------------
# the census
# ---------------------------------------------------------------------------------------------

def classify(x, ks=None):
    """Per block of ``x``: ``k``, ``kstar``, ``coded`` (param > 0), ``uw``, ``bw``, ``zero``, ``long``
    (uw >= 9) and ``canonical`` (what the encoder writes: k* or, for an all-zero block, param 0)."""
    W, zb, params, bw, S, words, kstar, zero = plan_forced(x, ks)
    coded = params > 0
    k = np.maximum(params.astype(np.int64) - 1, 0)
    uw = np.where(coded, bw.astype(np.int64) - 2 * k, 0)
    return dict(W=W, zb=zb, params=params.astype(np.int64), bw=bw.astype(np.int64), S=S, words=words, kstar=kstar,
                zero=zero, coded=coded, k=k, uw=uw, long=uw >= 9,
                canonical=np.where(zero, ~coded, coded & (k == kstar)))


def _walk_bit31(us, uw, pos):
    """The decoder's word walk over a lane's 8 codes (stream words ``us``, the lane starts at bit
    ``pos``): how often a terminator is met at bit 31 of the word in hand (``tz == 31``)."""
    wi, n31 = pos >> 5, 0
    cur = us[wi] >> (pos & 31) if wi < uw else 0
    base = pos
    for _ in range(8):
        while cur == 0 and wi + 1 < uw:
            wi += 1
            cur = us[wi]
            base = 32 * wi
        if cur == 0:
            break
        tz = (cur & -cur).bit_length() - 1
        n31 += tz == 31
        pos = base + tz + 1
        cur = 0 if tz == 31 else cur >> (tz + 1)
        base = pos
    return n31


def census(x, ks=None):
    """Counter of the paths the array reaches: blocks, lanes, samples or wave steps per bucket, as
    the bucket's name says.  Encoder buckets are counted on canonical blocks only, and the encoder's
    step buckets only when no k is forced (``ks is None``)."""
    x = np.ascontiguousarray(np.asarray(x).reshape(-1))
    c = Counter()
    f = classify(x, ks)
    W, zb, nb = f['W'], f['zb'], len(f['k'])
    if nb == 0:
        return c
    nstep = -(-nb // STEP)
    step_long = np.zeros(nstep, bool)
    np.logical_or.at(step_long, np.arange(nb) // STEP, f['coded'] & f['long'])
    for b in range(nb):
        k, uw, bw, kstar = int(f['k'][b]), int(f['uw'][b]), int(f['bw'][b]), int(f['kstar'][b])
        if not f['coded'][b]:
            c['zero block'] += 1
            continue
        canon = bool(f['canonical'][b])
        if canon:
            c[f'k*={k}'] += 1
            wd = f['words'][b, :W]
            mins = np.flatnonzero(wd == wd.min())
            if len(mins) > len(set((mins // 8).tolist())):
                c['tie in group'] += 1
            for g in (7, 15, 23):
                if g in mins and g + 1 in mins:
                    c[f'tie across {g}|{g + 1}'] += 1
            if bw == 2 * W + 2:
                c['bw=2W+2'] += 1
            if W == 32:
                for kk in (0, 8, 16):
                    if f['S'][b, kk] != CAP:
                        c[f'S{kk} {"above" if f["S"][b, kk] > CAP else "below"} cap, k* group {k // 8}'] += 1
        elif f['zero'][b]:
            c[f'forced: zero block coded k={k}'] += 1
        elif uw >= 9:
            c[f'forced: long k={k} uw={uw}'] += 1
            if uw == 2 * W + 2 - 2 * k:
                c[f'forced: long k={k} uw=max'] += 1
        else:
            if k > kstar:
                c['forced: k>k* short'] += 1
            if k == W - 1 and kstar <= 3:
                c['forced: k=W-1 small'] += 1
        q = (zb[b] >> np.uint64(k)).astype(np.int64)
        lens = 8 + q.reshape(8, 8).sum(axis=1)
        incl = np.cumsum(lens)
        term = np.cumsum(q + 1) - 1
        us = [0] * uw
        for t in term:
            us[int(t) >> 5] |= 1 << (int(t) & 31)
        if canon:
            c['code >=64 zeros'] += int((q >= 64).sum())
            c['code >=96 zeros'] += int((q >= 96).sum())
        for j in range(8):
            ln, p0 = int(lens[j]), int(incl[j] - lens[j])
            win = 'w32' if ln <= 32 else 'w64' if ln <= 64 else 'walk'
            c[f'dec lane {win}'] += 1
            if step_long[b // STEP]:
                c[f'long step lane {win}'] += 1
                if j > 0 and (p0 >> 5) >= 8:
                    c['long step lane start word>=8'] += 1
            if uw == 8 and j > 0 and p0 - 1 >= 224:
                c['uw=8, terminator 8j-1 in word 7'] += 1
            if not canon:
                continue
            if ln <= 32:
                c['enc lane one mask, ' + ('carry' if (p0 & 31) + ln > 32 else 'no carry')] += 1
            else:
                c['enc lane 33..64' if ln <= 64 else 'enc lane >64'] += 1
            if j > 0 and (p0 & 31) == 0:
                c[f'lane start aligned j={j}'] += 1
            if ln > 64:
                c['walk: terminator at bit 31'] += _walk_bit31(us, uw, p0)
    sv = np.zeros(nstep * STEP_SAMPLES, np.int64)
    sv[:x.size] = x.view(np.dtype(f'i{W // 8}')).astype(np.int64)
    sv = sv.reshape(nstep, STEP_SAMPLES)
    for s in range(nstep):
        sl = slice(STEP * s, min(nb, STEP * s + STEP))
        coded, params = f['coded'][sl], f['params'][sl]
        if STEP * s + STEP > nb:
            c['step tail past nb'] += 1
        if coded.any() and not coded.all():
            c['step zero+coded'] += 1
        if W >= 16 and ks is None:
            out = np.flatnonzero((sv[s] < -128) | (sv[s] > 127))
            if len(out) == 0:
                c['enc lo step'] += 1
                if (sv[s] == -128).any() and (sv[s] == 127).any():
                    c['enc lo step with -128 and 127'] += 1
            else:
                c['enc full step'] += 1
                if len(out) == 1 and int(out[0]) in (0, STEP_SAMPLES - 1) and int(sv[s, out[0]]) in (-129, 128):
                    c[f'enc full step, only sample {int(out[0])} = {int(sv[s, out[0]])}'] += 1
        lo8 = bool((params <= 9).all())
        if W >= 16:
            c['dec lo8 step' if lo8 else 'dec step not lo8'] += 1
            if not lo8 and (coded & (f['k'][sl] <= 8)).any():
                c['dec step not lo8 with k<=8'] += 1
        if not step_long[s]:
            c['dec short step'] += 1
            continue
        c['dec long step'] += 1
        lg = f['long'][sl] & coded
        if W >= 16 and not lo8:
            c['long step not lo8'] += 1
        if lg[coded].all():
            c['long step, every coded block long'] += 1
        if lg.sum() == 1 and len(lg) == STEP and f['canonical'][sl][~lg].all() and not coded.all():
            c[f'long step, one long block at {int(np.flatnonzero(lg)[0])}, 7 canonical'] += 1
    return c


def long_combos(W):
    """The ``(k, uw)`` of the long blocks asked for: uw in {9, 16, 17} where the format allows it and
    the largest it allows, 2W + 2 - 2k, at k = 0, 3 and (W >= 16, so that the step is not lo8) 9."""
    out = []
    for k in (0, 3, 9):
        if k == 9 and W < 16:
            continue
        top = 2 * W + 2 - 2 * k
        out += [(k, u) for u in (9, 16, 17) if u < top] + [(k, top)]
    return out


def required_reach(W):
    """Buckets that data packed by the kernels (k* everywhere) must reach."""
    r = [f'k*={k}' for k in range(W)] + ['tie in group']
    r += [f'tie across {g}|{g + 1}' for g in (7, 15, 23) if g + 1 < W]
    r += ['zero block', 'step zero+coded', 'step tail past nb']
    if W >= 16:
        r += ['enc lo step', 'enc full step', 'enc lo step with -128 and 127', 'dec lo8 step',
              'dec step not lo8 with k<=8']
        r += [f'enc full step, only sample {p} = {v}' for p in (0, STEP_SAMPLES - 1) for v in (-129, 128)]
    if W == 32:
        # S_k above the cap needs z of about 2^(k + 14) and more, which puts k* into the groups from
        # (k + 14) // 8 up; every other pair of {k = 0, 8, 16} x {below, above} x {group} is here
        r += [f'S{kk} above cap, k* group {g}' for kk, gs in ((0, (1, 2, 3)), (8, (2, 3)), (16, (3,))) for g in gs]
        r += [f'S{kk} below cap, k* group {g}' for kk, gs in ((0, (0, 1)), (8, (0, 1, 2)), (16, (0, 1, 2, 3)))
              for g in gs]
    r += ['enc lane one mask, no carry', 'enc lane one mask, carry', 'enc lane 33..64', 'enc lane >64',
          'dec lane w32', 'dec lane w64', 'dec lane walk',
          'code >=64 zeros', 'code >=96 zeros', 'walk: terminator at bit 31']
    r += [f'lane start aligned j={j}' for j in range(1, 8)]
    r += ['bw=2W+2', 'dec short step']
    return r


def required_forced(W):
    """Buckets that only a forced k reaches (valid by the format, written by no encoder)."""
    r = ['dec long step', 'long step, every coded block long']
    r += [f'long step, one long block at {g}, 7 canonical' for g in range(STEP)]
    for k, u in long_combos(W):
        r.append(f'forced: long k={k} uw=max' if u == 2 * W + 2 - 2 * k else f'forced: long k={k} uw={u}')
    r += ['long step lane w32', 'long step lane w64', 'long step lane walk', 'long step lane start word>=8']
    r += ['forced: zero block coded k=0', 'forced: k>k* short', 'forced: k=W-1 small',
          'uw=8, terminator 8j-1 in word 7']
    if W >= 16:
        r.append('long step not lo8')
    return r


def format_census(c, names):
    return ', '.join(f'{n}: {c.get(n, 0)}' for n in names)


# ---------------------------------------------------------------------------------------------
# generators: blocks (uint64[64], zigzag domain) built from a target
# ---------------------------------------------------------------------------------------------

def _rng(*key):
    return np.random.default_rng([int(v) for v in key])


def kstar_of(z, W):
    return int(np.argmin(tables(np.asarray(z, np.uint64).reshape(1, BLOCK), W)[1][0]))


def _spread(rng, total, where):
    """``total`` units thrown at the sample positions ``where``: int64[64] quotients."""
    where = np.asarray(where)
    return np.bincount(where[rng.integers(0, len(where), total)], minlength=BLOCK).astype(np.int64)


def zero_block():
    return np.zeros(BLOCK, np.uint64)


def quot_block(W, K, q, rng):
    """k* = K with the quotients ``q`` at K: 17 <= sum(q) <= 64 and bit K - 1 set in every sample.
    words(K) = 2K + 3 or 2K + 4; S_{K-1} = 2 S_K + 64 >= 98 makes words(K - 1) >= 2K + 4 (+ 1 for
    S_K > 32), S_{K+1} <= 32 makes words(K + 1) >= 2K + 4: no smaller k ties, a larger one may."""
    q = np.asarray(q, np.int64)
    assert 17 <= q.sum() <= 64 and q.max() < (1 << (W - K)), (K, int(q.sum()), int(q.max()))
    z = q.astype(np.uint64) << np.uint64(K)
    if K > 0:
        z |= np.uint64(1 << (K - 1))
    if K > 1:
        z |= rng.integers(0, 1 << (K - 1), BLOCK, dtype=np.uint64)
    assert kstar_of(z, W) == K
    return z


def kstar_block(W, K, rng):
    """k* = K: 32 samples with quotient 1, no tie."""
    q = np.zeros(BLOCK, np.int64)
    q[rng.permutation(BLOCK)[:32]] = 1
    return quot_block(W, K, q, rng)


def lane_block(W, K, j, lane_total, rest_total, rng):
    """k* = K with lane j's 8 codes ``8 + lane_total`` bits long and ``rest_total`` spread elsewhere."""
    lane = np.arange(8 * j, 8 * j + 8)
    q = _spread(rng, lane_total, lane) + _spread(rng, rest_total, np.setdiff1d(np.arange(BLOCK), lane))
    return quot_block(W, K, q, rng)


def tie_block(W, b, rng):
    """words(k) minimal at k = b, b + 1 and b + 2: z in [2^(b+1), 2^(b+1) + 2^b) gives quotients
    2, 1, 0 there (2b + 6 words each) and >= 4 at b - 1 (2b + 8)."""
    assert 0 <= b <= W - 2
    z = np.uint64(1 << (b + 1)) + rng.integers(0, 1 << b, BLOCK, dtype=np.uint64)
    assert kstar_of(z, W) == b
    return z


def spike_block(W, K, q, pos, rng):
    """One sample with quotient q in [81, 128] at K, the rest zero: k* = K (words(K) = 2K + 5 or
    2K + 6; K - 1 needs two words more for the code and saves two planes less one; K + 1 ties at
    best)."""
    assert 81 <= q <= 128 and q < (1 << (W - K))
    z = np.zeros(BLOCK, np.uint64)
    z[pos] = (q << K) | (int(rng.integers(0, 1 << K)) if K else 0)
    assert kstar_of(z, W) == K
    return z


def aligned_block(W, K, j, rng):
    """Lane j starts at a stream bit that is a multiple of 32: the lanes before it hold 8j
    terminators and one quotient (-8j) mod 32, the lanes from j on 20 units."""
    q = _spread(rng, 20, np.arange(8 * j, BLOCK))
    q[0] = (-8 * j) % 32
    z = quot_block(W, K, q, rng)
    return z


def full_block(W, rng):
    """bw = 2W + 2, the most a block can take: the two top bits of every z set."""
    z = np.uint64(3 << (W - 2)) | rng.integers(0, 1 << (W - 2), BLOCK, dtype=np.uint64)
    assert tables(z.reshape(1, BLOCK), W)[1][0].min() == 2 * W + 2
    return z


def zz(v):
    v = np.asarray(v, np.int64)
    return np.where(v >= 0, 2 * v, -2 * v - 1).astype(np.uint64)


def filler_blocks(nblk, rng, scale=1.5):
    """Small Laplacian residuals (the usual map)."""
    return list(zz(np.rint(rng.laplace(0.0, scale, nblk * BLOCK))).reshape(nblk, BLOCK))


def lo_step(rng, extremes=False, out=None):
    """A wave step of residuals in [-100, 100]; ``extremes``: -128 and 127 among them; ``out = (sample,
    value)``: that one sample set to a value just outside [-128, 127]."""
    v = np.clip(np.rint(rng.laplace(0.0, 20.0, STEP_SAMPLES)), -100, 100).astype(np.int64)
    if extremes:
        p = rng.permutation(STEP_SAMPLES)[:4]
        v[p] = (-128, 127, -128, 127)
    if out is not None:
        v[out[0]] = out[1]
    return list(zz(v).reshape(STEP, BLOCK))


def long_block(W, k, uw, rng):
    """A block that takes ``uw`` unary words at the forced k (no encoder writes uw >= 8): quotients
    summing to 32 uw - 64 - r, r < 32, a quarter each on three samples, the rest spread."""
    qmax = (1 << (W - k)) - 1
    S = 32 * uw - 64 - int(rng.integers(0, 32))
    heavy = rng.permutation(BLOCK)[:3]
    q = np.zeros(BLOCK, np.int64)
    q[heavy] = min(S // 4, qmax)
    q += _spread(rng, S - int(q.sum()), np.setdiff1d(np.arange(BLOCK), heavy))
    assert q.max() <= qmax and (64 + q.sum() + 31) // 32 == uw
    z = q.astype(np.uint64) << np.uint64(k)
    if k:
        z |= rng.integers(0, 1 << k, BLOCK, dtype=np.uint64)
    return z


def word7_block(jj, rng):
    """uw = 8 at k = 0 with terminator 8 jj - 1 (jj = 5, 6, 7) in stream word 7: the samples before
    lane jj hold 225 - 8 jj .. 232 - 8 jj quotient units, the others none."""
    assert 5 <= jj <= 7
    q = _spread(rng, 225 - 8 * jj + int(rng.integers(0, 8)), np.arange(8 * jj))
    assert 161 <= q.sum() <= 192
    return q.astype(np.uint64)


def to_samples(blocks, dtype, n):
    """The first ``n`` samples of the z blocks as ``dtype`` bit patterns."""
    W = sample_bits(dtype)
    z = np.concatenate(blocks) if len(blocks) else np.zeros(0, np.uint64)
    return unzigzag(z[:n], W).view(np.dtype(dtype))


def _sized(blocks, kind, rng):
    """``blocks`` (whole steps) followed by filler so that the array ends on size kind ``kind``:
    ``(blocks, n)``."""
    nc = len(blocks)
    assert nc % STEP == 0 and nc + STEP < R.TILE_BLOCKS
    if kind >= 6:
        fill = R.TILE_BLOCKS + 1 - nc
        n = TILE_SAMPLES + (kind - 6)
    else:
        fill = STEP + 1
        n = (64 * (nc + 5) + 24, 64 * (nc + 5) + 25, 64 * (nc + 3), 64 * (nc + 3) + 1, 64 * (nc + 8),
             64 * (nc + 8) + 1)[kind]
    return blocks + filler_blocks(fill, rng), n


def _small_array(W, i, dtype, rng):
    """1 .. 7 blocks with a ragged end: a step whose tail blocks lie past nb."""
    nbk = 1 + i % 7
    blocks = filler_blocks(nbk, rng, 3.0)
    if nbk > 2:
        blocks[1] = zero_block()
    return to_samples(blocks, dtype, 64 * nbk - 3 - 2 * (i % 4))


def _lane_k(W, need_bits, rng):
    return int(rng.integers(0, W - need_bits + 1))


def reach_bundle(W, i):
    """Bundle i (0 .. 7) of encoder-reachable arrays of W-bit samples: ``[main, small]``."""
    rng = _rng(W, i, 1)
    dts = DTYPES[W]
    steps = []
    # every k*, interleaved so that (W >= 16) each step holds k <= 8 and k >= 9
    for s in range(W // 8):
        steps.append([kstar_block(W, K, rng) for K in range(s, W, W // 8)])
    # ties inside a plane group and across each group boundary; zero blocks among coded ones
    inner = [b for b in range(W - 1) if b % 8 != 7]
    cross = [b for b in (7, 15, 23) if b <= W - 2]
    bs = cross + [inner[(i + 3 * t) % len(inner)] for t in range(6 - len(cross))]
    tie = [tie_block(W, b, rng) for b in bs]
    steps.append([tie[0], zero_block(), tie[1], tie[2], zero_block(), tie[3], tie[4], tie[5]])
    if W >= 16:
        steps.append(lo_step(rng))
        steps.append(lo_step(rng, extremes=True))
        steps += [lo_step(rng, out=(p, v)) for p in (0, STEP_SAMPLES - 1) for v in (-129, 128)]
    # lanes: short codes, 33 .. 64 bits, past 64 bits (a different lane in every bundle), one code of
    # 81 .. 95 zeros ending on bit 31 of stream word 2, one of 96 .. 127 zeros
    p31 = (2 * i + 1) % 15
    steps.append([
        quot_block(W, _lane_k(W, 3, rng), _spread(rng, 24, np.arange(BLOCK)), rng),
        quot_block(W, _lane_k(W, 3, rng), _spread(rng, 40, np.arange(BLOCK)), rng),
        lane_block(W, _lane_k(W, 5, rng), i % 8, 26 + i, 10, rng),
        lane_block(W, _lane_k(W, 5, rng), (i + 3) % 8, 40 - i, 8, rng),
        lane_block(W, _lane_k(W, 6, rng), (i + 1) % 8, 58, 3, rng),
        lane_block(W, _lane_k(W, 6, rng), (i + 5) % 8, 60, 2, rng),
        spike_block(W, _lane_k(W, 7, rng), 95 - p31, p31, rng),
        spike_block(W, _lane_k(W, 7, rng), 96 + (5 * i) % 32, int(rng.integers(0, BLOCK)), rng)])
    # lane j starting on a word boundary, j = 1 .. 7
    steps.append([aligned_block(W, _lane_k(W, 5, rng), j, rng) for j in range(1, 8)] + [zero_block()])
    # the largest block, and a second code ending on bit 31 of stream word 2 (after 7 + i terminators)
    p31 = 7 + i
    steps.append([full_block(W, rng), kstar_block(W, i % W, rng), full_block(W, rng), zero_block(),
                  spike_block(W, _lane_k(W, 7, rng), 95 - p31, p31, rng),
                  lane_block(W, _lane_k(W, 5, rng), 7 - i % 8, 30, 12, rng),
                  quot_block(W, _lane_k(W, 3, rng), _spread(rng, 50, np.arange(BLOCK)), rng), zero_block()])
    blocks, n = _sized([b for st in steps for b in st], i, rng)
    return [to_samples(blocks, dts[i % len(dts)], n), _small_array(W, i, dts[(i + 1) % len(dts)], rng)]


def forced_bundle(W, i):
    """Bundle i (0 .. 7) with forced parameters: ``([main, small], [ks of main, None])``.  ``main``:
    two steps of long blocks only, one step per group position with one long block among seven
    canonical ones, one step of non-canonical short blocks, then filler up to size kind i."""
    rng = _rng(W, i, 2)
    dts = DTYPES[W]
    combos = long_combos(W)
    blocks, ks = [], []

    def add(z, k=None):
        blocks.append(z)
        ks.append(k)

    for t in range(2 * STEP):  # every (k, uw) at least once
        k, u = combos[(t + i) % len(combos)] if t >= len(combos) else combos[t]
        add(long_block(W, k, u, rng), k)
    for g in range(STEP):
        zpos = (g + 1 + i % 7) % STEP
        for p in range(STEP):
            if p == g:
                k, u = combos[(g + i) % len(combos)]
                add(long_block(W, k, u, rng), k)
            elif p == zpos:
                add(zero_block())
            elif p % 3 == 0:
                add(kstar_block(W, int(rng.integers(0, W)), rng))
            elif p % 3 == 1:
                add(lane_block(W, _lane_k(W, 6, rng), int(rng.integers(0, 8)), 40 + 2 * p, 4, rng))
            else:
                add(quot_block(W, _lane_k(W, 3, rng), _spread(rng, 30, np.arange(BLOCK)), rng))
    K = _lane_k(W, 5, rng)
    add(zero_block(), 0)                                                  # an all-zero block coded with k = 0
    add(quot_block(W, K, _spread(rng, 40, np.arange(BLOCK)), rng), K + 2)  # k > k*
    add(filler_blocks(1, rng, 3.0)[0], W - 1)                             # k = W - 1 on small residuals
    add(word7_block(5 + i % 3, rng), 0)
    add(filler_blocks(1, rng, 2.0)[0], W - 1)
    add(zero_block(), -1)
    add(zero_block(), 0)
    add(word7_block(5 + (i + 1) % 3, rng), 0)
    blocks, n = _sized(blocks, i, rng)
    ks += [None] * (-(-n // BLOCK) - len(ks))
    return ([to_samples(blocks, dts[(i + 1) % len(dts)], n), _small_array(W, i, dts[i % len(dts)], rng)],
            [ks[:-(-n // BLOCK)], None])


def sparse_tiles(ntile, dtype, seed):
    """``ntile`` tiles of mostly zero blocks with 1 .. 7 coded blocks each, of a k* and a count that
    change from tile to tile, so that no two neighbouring tiles have the same word count."""
    W = sample_bits(dtype)
    rng = _rng(W, ntile, seed)
    z = np.zeros((ntile * R.TILE_BLOCKS, BLOCK), np.uint64)
    for t in range(ntile):
        for c in range(1 + t % 7):
            z[t * R.TILE_BLOCKS + int(rng.integers(0, R.TILE_BLOCKS))] = kstar_block(W, (t + 3 * c) % W, rng)
    return unzigzag(z.reshape(-1), W).view(np.dtype(dtype))
