"""Test infrastructure for the categorical rank coder (numpy only: neither torch nor the library).

``decode_path`` / ``encode_path`` restate the *control flow* of the vector kernels of
``kmp_categorical.hip`` -- which key path, peel or radix select, how many maxima or rounds, owner
slot or tie walk; packed-count fast path or ballot fallback -- and name the bucket an element falls
into next to the answer.  They say nothing about lanes, LDS or the prefetch ring.  ``range_plan``
restates the host rule that hands each wave a contiguous range of elements.  The generators build
rows from bit patterns, so the number P of low bits in which a row's keys differ is set by
construction, and the census of buckets they reach is a condition the CPU suite asserts
(``test_categorical_spec.py``) before the GPU suite relies on it.
"""

import numpy as np

RAW_BASE = 0x3f000000    # 0.5: every logit non-negative, the decode's raw-bits key path
ORDER_BASE = 0xbf000000  # -0.5: every logit negative, the order-key path
BASES = (('raw', RAW_BASE), ('order', ORDER_BASE))
SPREADS = (0, 1, 3, 8, 9, 12, 16, 17, 20, 24, 25, 30)  # m: offsets below 2^m
PAIR_SPREADS = (12, 16, 20, 24, 25, 30)
LONELY_SPREADS = (4, 8, 12, 16, 20, 24, 30)
CLUSTER_WIDTHS = (8, 16, 24)
PEEL = 4        # kCatPeel: decode ranks below this peel maxima
WAVES = 4       # kCatWaves
PATH_LS = (8, 64, 252, 256, 300, 512)
CENSUS_LS = tuple(L for L in PATH_LS if L >= 64)

PEEL_BUCKETS = tuple(('peel', mx, end) for mx in (1, 2, 3, 4) for end in ('one', 'ties'))
RADIX_BUCKETS = (('radix', 0, 1, 'ties'),) + tuple(
    b for c in (1, 2, 3, 4) for b in dict.fromkeys(
        (('radix', c, 1, 'owner'), ('radix', c, c, 'owner'), ('radix', c, c, 'ties'))))
REQUIRED_DECODE = tuple((kp,) + b for kp in ('raw', 'order') for b in PEEL_BUCKETS + RADIX_BUCKETS)
ENCODE_BUCKETS = ('none', 'fast', 'ties', 'nan', 'alias')


def ranks_for(L):
    """The ranks every generated row is decoded at (and the values it is encoded with)."""
    return (0, 1, 2, 3, 4, 5, L // 2, L - 1, L + 2)


# ---------------------------------------------------------------------------------------------
# The path model
# ---------------------------------------------------------------------------------------------

def decode_keys(row, L):
    """``(keypath, keys)``: raw float bits (+1 unless every class of the vector slot exists, L 256
    or 512) when no logit's bits exceed +inf's; else the order key (-0 -> +0, negatives inverted,
    every NaN -> 0xffffffff)."""
    row = np.ascontiguousarray(row, dtype=np.float32)
    bits = row.view(np.uint32).astype(np.int64)
    if (bits <= 0x7f800000).all():
        return 'raw', bits + (0 if L in (256, 512) else 1)
    u = np.where(row == 0, np.float32(0), row).view(np.uint32).astype(np.int64)
    keys = np.where(u & 0x80000000, u ^ 0xffffffff, u | 0x80000000)
    keys[np.isnan(row)] = 0xffffffff
    return 'order', keys


def _mth_highest(idx, m):
    return int(np.sort(idx)[::-1][m])


def decode_path(row, value, L):
    """``(bucket, class)`` of the decode of rank ``value`` (any integer) on one row of L logits."""
    assert len(row) == L
    kp, keys = decode_keys(row, L)
    k = min(max(int(value), 0), L - 1)
    if k < PEEL:
        taken = 0
        for mx, wmax in enumerate(np.unique(keys)[::-1], 1):
            idx = np.flatnonzero(keys == wmax)
            if taken + len(idx) > k:
                return (kp, 'peel', mx, 'one' if len(idx) == 1 else 'ties'), _mth_highest(idx, k - taken)
            taken += len(idx)
        raise AssertionError('peel ran out of keys')
    dif = int(np.bitwise_or.reduce(keys ^ keys[0]))
    P = dif.bit_length()
    c = (P + 7) // 8
    sh = max(P - 8, 0)
    wd = P - sh
    inside = np.ones(L, dtype=bool)
    c_hi, rounds = 0, 0
    while True:
        rounds += 1
        digit = (keys >> sh) & ((1 << wd) - 1)
        counts = np.bincount(digit[inside], minlength=256)
        r, cb, d = k - c_hi, 0, (1 << wd) - 1
        while r >= cb + counts[d]:  # bins in descending digit order
            cb += int(counts[d])
            d -= 1
        c_hi += cb
        cnt = int(counts[d])
        inside &= digit == d
        if cnt > 1 and sh != 0:
            nsh = max(sh - 8, 0)
            wd, sh = sh - nsh, nsh
            continue
        break
    idx = np.flatnonzero(inside)
    assert len(idx) == cnt and cnt >= 1
    if cnt == 1:
        return (kp, 'radix', c, rounds, 'owner'), int(idx[0])
    return (kp, 'radix', c, rounds, 'ties'), _mth_highest(idx, k - c_hi)


def encode_path(row, value, L, bits):
    """``(bucket, code)`` of the encode of class ``value`` (any integer) in a ``bits``-wide value
    dtype: the smallest descending rank among the classes that match modulo 2^bits, 0 if none."""
    assert len(row) == L
    row = np.asarray(row, dtype=np.float32)
    g = int(value)
    cands = list(range(g, L, 1 << bits)) if g >= 0 else []
    if not cands:
        return 'none', 0
    nan = np.isnan(row)
    best = None
    for i in cands:
        li = row[i]
        j = np.arange(L)
        if nan[i]:
            before = ~nan | (nan & (j < i))
        else:
            with np.errstate(invalid='ignore'):
                before = (row < li) | ((row == li) & (j < i))
        p = L - 1 - int(before.sum())
        best = p if best is None else min(best, p)
    code = best & ((1 << bits) - 1)
    if len(cands) > 1:
        return 'alias', code
    i = cands[0]
    if nan[i]:
        return 'nan', code
    return ('fast' if int((row == row[i]).sum()) == 1 else 'ties'), code


def range_plan(n, L):
    """``(per, lengths)``: the vector kernel's elements per wave and every wave's range length
    (the host rule of ``kmp_categorical``: 2 048 blocks of 4 waves at the most, more only to keep a
    wave's rows below 2^31 bytes)."""
    g = -(-n // WAVES)
    per_max = (1 << 31) // (L * 4) - 1
    g_min = -(-n // (per_max * WAVES))
    vgrid = max(min(g, 2048), g_min)
    nw = WAVES * vgrid
    per = -(-n // nw)
    return per, [max(0, min(n, (w + 1) * per) - w * per) for w in range(nw)]


def ring_tail(length, pf=4):
    """``(main_rounds, left)``: rounds of the prefetch ring's main loop over a range of ``length``
    elements and the elements left for the two tail loops."""
    if length < 2 * pf:
        return 0, length
    rounds = (length - 2 * pf) // pf + 1
    return rounds, length - rounds * pf


def range_sizes(lo=2, hi=12):
    """The element counts of the range-length tests at L = 8."""
    return [8192 * per - r for per in range(lo, hi + 1) for r in (0, 1, 5)] + [8193]


# ---------------------------------------------------------------------------------------------
# Generators: rows from bit patterns
# ---------------------------------------------------------------------------------------------

def _f32(bits):
    return np.asarray(bits, dtype=np.int64).astype(np.uint32).view(np.float32)


def _distinct(rng, hi, count):
    """``count`` distinct integers below ``hi`` (plain draws when there are not that many)."""
    if hi < count:
        return rng.integers(0, max(hi, 1), count)
    if hi <= 1 << 16:
        return rng.permutation(hi)[:count]
    v = np.unique(rng.integers(0, hi, count))
    while len(v) < count:
        v = np.unique(np.concatenate([v, rng.integers(0, hi, count)]))
    return rng.permutation(v)[:count]


def _pin_top(rng, off, m, L):
    """Two classes at offsets 0 and 2^(m-1): with every other offset below 2^m - 1 the keys differ in
    exactly the m low bits, with and without the raw path's + 1."""
    if m >= 1 and L >= 2:
        i0, i1 = rng.permutation(L)[:2]
        off[i0], off[i1] = 0, 1 << (m - 1)
    return off


def spread_row(rng, L, base, m, distinct):
    """Offsets below 2^m on ``base``: P == m.  ``distinct``: no two classes equal (while 2^m
    allows); otherwise three offsets shared by all classes (long tie runs)."""
    hi = (1 << m) - 1 if m >= 2 else 1 << m  # 2^m - 1 itself would carry into bit m on the + 1
    if distinct:
        off = np.asarray(_distinct(rng, hi, L), dtype=np.int64)
        if m >= 1 and L >= 2 and hi >= L + 2:  # keep them distinct around the two pinned offsets
            off = off[(off != 0) & (off != 1 << (m - 1))]
            while len(off) < L:
                v = int(rng.integers(0, hi))
                if v != 0 and v != 1 << (m - 1) and v not in off:
                    off = np.append(off, v)
            off = off[:L]
            i0, i1 = rng.permutation(L)[:2]
            off[i0], off[i1] = 0, 1 << (m - 1)
        else:
            off = _pin_top(rng, off, m, L)
    else:
        vals = np.array([0, (1 << (m - 1)) if m >= 1 else 0, int(rng.integers(0, hi))], dtype=np.int64)
        off = vals[rng.integers(0, 3, L)]
        off[rng.permutation(L)[:min(3, L)]] = vals[:min(3, L)]
    if m == 1 and base == RAW_BASE and L not in (256, 512):
        off = off + 1  # the raw path's + 1 then makes the keys base + {2, 3}: one differing bit
    return _f32(base + off)


def cluster_row(rng, L, width, order, tied):
    """A cluster ``width`` bits wide at 0.5 plus two far outliers -- a denormal and, for the order
    path, -1.0 (P == 32), for the raw path 2^127 (P == 31): the first rounds see the whole cluster in
    one bin.  ``tied``: a third of the classes equal class 0."""
    bits = RAW_BASE + np.asarray(_distinct(rng, 1 << width, L), dtype=np.int64)
    if tied:
        bits[rng.permutation(np.arange(1, L))[:max(L // 3, 1)]] = bits[0]
    o0, o1 = rng.permutation(np.arange(1, L))[:2]
    bits[o0] = 0x00000123
    bits[o1] = 0xbf800000 if order else 0x7f000000
    return _f32(bits)


def pair_row(rng, L, base, m):
    """Pairs of classes that differ only in their low four bits inside a spread of m bits: the
    select has to go down to the last digit and ends on a single key (the owner slot)."""
    half = (L + 1) // 2
    hi = ((1 << m) - 1) >> 4
    stem = np.asarray(_distinct(rng, hi, half), dtype=np.int64) << 4
    stem = _pin_top(rng, stem, m, half)
    lo = np.array([rng.permutation(15)[:2] for _ in range(half)], dtype=np.int64)  # <= 14: the + 1 never carries
    off = np.concatenate([stem + lo[:, 0], stem + lo[:, 1]])[:L]
    return _f32(base + off[rng.permutation(L)])


def lonely_row(rng, L, base, m):
    """Six classes alone in their first-round bins (the six largest first digits) above two long tie
    runs at offsets 2^(m-1) and 0: ranks 0..3 peel one key each, ranks 4 and 5 end the radix select on
    an owner slot in its first round, however many classes there are."""
    wd = min(m, 8)
    low = m - wd
    digit = (1 << wd) - 2 - np.arange(6, dtype=np.int64)
    single = (digit << low) + (rng.integers(0, (1 << low) - 1, 6) if low >= 2 else 0)
    off = np.where(rng.integers(0, 2, L) == 1, 1 << (m - 1), 0).astype(np.int64)
    off[:2] = [0, 1 << (m - 1)]
    off[rng.permutation(np.arange(2, L))[:6]] = single[:max(min(6, L - 2), 0)]
    bits = base + off
    if base & 0x80000000:
        bits = base + ((1 << m) - off)
    return _f32(bits)


def ladder_row(rng, L, base, singles):
    """``singles`` distinct largest logits, then three classes tied, then distinct smaller ones: the
    peel takes ``singles + 1`` maxima and ends in a tie."""
    off = np.asarray(_distinct(rng, 1 << 16, L), dtype=np.int64)
    top = (1 << 20) + 16 * np.array([0, 0, 0] + list(range(1, singles + 1)), dtype=np.int64)
    pos = rng.permutation(L)[:min(len(top), L)]
    off[pos] = top[:len(pos)]
    bits = base + off
    if base & 0x80000000:  # negative floats: larger magnitude sorts lower
        bits = base + ((1 << 21) - off)
    return _f32(bits)


def special_rows(rng, L):
    """Denormals, infinities, signed zeros, NaNs of either sign and several payloads, an all-NaN
    row, all-equal rows."""
    def tile(vals, dtype=np.float32):
        return np.resize(np.asarray(vals, dtype=dtype), L)

    def sprinkle(row, bits):
        row = row.copy()
        u = row.view(np.uint32)
        for i, b in enumerate(bits):
            u[i % L] = b
            u[(L - 1 - 2 * i) % L] = b
        return row

    rnd = rng.random(L).astype(np.float32)
    nrm = rng.standard_normal(L).astype(np.float32)
    den = [0.0, 1e-45, 3e-45, 1e-40, 1e-39]
    nans = [0x7fc00000, 0xffc00000, 0x7f800001, 0xffffffff, 0x7fc12345]
    rows = [
        ('denormal+', tile(den)),
        ('denormal+-', tile(den + [-1e-45, -3e-45, -1e-40, -1e-39, -0.0])),
        ('denormal-', -tile(den[1:])),
        ('denormal in softmax', sprinkle(rnd, [0x00000001, 0x00000002, 0x00012345, 0x007fffff, 0x00800000])),
        ('inf+', sprinkle(rnd, [0x7f800000, 0x7f800000, 0x00000000])),
        ('inf+-', sprinkle(nrm, [0x7f800000, 0xff800000, 0x7f800000, 0xff800000])),
        ('zeros', tile([-0.0, 0.0])),
        ('zeros and quarters', tile([-0.0, 0.0, 0.25, -0.25, 0.0, -0.0, 0.25])),
        ('nan payloads', sprinkle(nrm, nans)),
        ('nan in softmax', sprinkle(rnd, nans[:3])),
        ('all nan', tile(nans, np.uint32).view(np.float32)),
        ('all +0.5', tile([0.5])),
        ('all -0.5', tile([-0.5])),
        ('all +0', tile([0.0])),
        ('all -0', tile([-0.0])),
    ]
    return rows


_CACHE = {}


def rows(L, seed=0):
    """``(logits[R, L] float32, tags)``: every generated row at L classes, seeded."""
    if (L, seed) in _CACHE:
        return _CACHE[L, seed]
    rng = np.random.default_rng([seed, L])
    out = []
    for kp, base in BASES:
        for m in SPREADS:
            for distinct in (True, False):
                for rep in range(3):
                    out.append((f'{kp} spread m={m} {"distinct" if distinct else "three values"}',
                                spread_row(rng, L, base, m, distinct)))
        for m in PAIR_SPREADS:
            for rep in range(3):
                out.append((f'{kp} pairs m={m}', pair_row(rng, L, base, m)))
        for m in LONELY_SPREADS:
            for rep in range(2):
                out.append((f'{kp} lonely m={m}', lonely_row(rng, L, base, m)))
        for singles in range(4):
            for rep in range(6):
                out.append((f'{kp} ladder {singles} singles', ladder_row(rng, L, base, singles)))
    for width in CLUSTER_WIDTHS:
        for order in (False, True):
            for tied in (False, True):
                for rep in range(3):
                    out.append((f'{"order" if order else "raw"} cluster width={width}{" tied" if tied else ""}',
                                cluster_row(rng, L, width, order, tied)))
    out += special_rows(rng, L)
    logits = np.stack([r for _, r in out]).astype(np.float32)
    logits.setflags(write=False)
    _CACHE[L, seed] = logits, [t for t, _ in out]
    return _CACHE[L, seed]


def elements(L, seed=0):
    """``(logits[N, L], ranks[N] int64, tags)``: every generated row once per rank of ``ranks_for``."""
    lg, tags = rows(L, seed)
    rk = np.asarray(ranks_for(L), dtype=np.int64)
    return np.repeat(lg, len(rk), axis=0), np.tile(rk, len(lg)), [t for t in tags for _ in rk]


def wrap(values, dtype):
    """Integers as the value dtype holds them (two's-complement wrap)."""
    return np.asarray(values, dtype=np.int64).astype(dtype)


def decode_census(L, dtype=np.int64, seed=0):
    """Bucket -> count over ``elements(L)`` with the ranks held in ``dtype``."""
    lg, rk, _ = elements(L, seed)
    census = {}
    for row, v in zip(lg, wrap(rk, dtype)):
        b = decode_path(row, int(v), L)[0]
        census[b] = census.get(b, 0) + 1
    return census


def encode_census(L, dtype, seed=0):
    lg, rk, _ = elements(L, seed)
    bits = 8 * np.dtype(dtype).itemsize
    census = {}
    for row, v in zip(lg, wrap(rk, dtype)):
        b = encode_path(row, int(v), L, bits)[0]
        census[b] = census.get(b, 0) + 1
    return census


def format_census(census):
    return ', '.join(f'{"/".join(map(str, b)) if isinstance(b, tuple) else b}: {n}'
                     for b, n in sorted(census.items(), key=lambda kv: str(kv[0])))


def alternating(L, seed=0):
    """``(logits[M, L], ranks[M])``: generated (row, rank) elements in an order that cycles peel,
    one-round radix, multi-round radix and tie elements, so a wave that ranks consecutive elements
    takes a different branch each time."""
    if ('alt', L, seed) in _CACHE:
        return _CACHE['alt', L, seed]
    lg, rk, _ = elements(L, seed)
    groups = [[], [], [], []]
    for i, (row, v) in enumerate(zip(lg, rk)):
        b = decode_path(row, int(v), L)[0]
        if b[-1] == 'ties':
            groups[3].append(i)
        elif b[1] == 'peel':
            groups[0].append(i)
        else:
            groups[1 if b[3] == 1 else 2].append(i)
    assert all(groups), [len(g) for g in groups]
    rng = np.random.default_rng([seed, L, 1])
    groups = [rng.permutation(g) for g in groups]
    M = 4 * max(len(g) for g in groups) + 3  # + 3: the cycle does not line up with the ring of 4
    idx = np.array([groups[i % 4][(i // 4) % len(groups[i % 4])] for i in range(M)])
    _CACHE['alt', L, seed] = lg[idx], rk[idx]
    return _CACHE['alt', L, seed]
