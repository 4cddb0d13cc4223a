"""The LinearPredictor's cast, as a specification: predictors whose predictions sit at the places
where the hand-written casts of the kernels could disagree (below zero, at and past the sample
maximum, at and past 2^32, infinite, NaN), and the cells every path must give for them.  Shared by
test_linear_cast_spec.py (the conditions, from the oracle alone) and test_gpu_linear_casts.py (the
kernels).  Pure numpy + oracle; knows nothing of the product.

A weight set gives each of the K channels one *class*:

``('const', name, c)``
    a zero weight column and bias ``c``: the value is exactly ``c`` in either arithmetic (the
    accumulator starts at the bias in float32 and every product is ``0 * f``), so the cell is
    ``cast_from_f32(c)`` with no tolerance.  Non-finite biases stand on these columns only.
``('sat', s)``
    a noisy-mean column (weights summing to 1) with bias ``s * max``, ``s`` = -1.2 or +1.2: every
    cell lies beyond the range by more than the 1e-5 (sum |f||w| + |b|) that bounds either arithmetic's
    distance from the float64 value, so the cell is 0 or max in both.
``('cross', s)``
    the same column with bias ``s * max`` for ``s`` in -0.5, 0, +0.5: predictions on both sides of a
    range edge.  Pinned to the oracle's fma chain for arith='f32'; for 'bf16x2', whose in-range bits the
    oracle does not restate, undecided here and compared across paths only.

The classes rotate cyclically over the channels, one weight set per rotation, so every channel
(a fixed lane, tile column or row position in a fused kernel) meets every class."""

import numpy as np

import oracle
from oracle import predictors as OP
from oracle.common import cast_from_f32

NPRED = {3: 19, 2: 5}
MARGIN = 1e-5  # the bound of tests/test_gpu_linear.py on |kernel f32 - float64| / (sum |f||w| + |b|)


def ons(ndim):
    return oracle.volume if ndim == 3 else oracle.image


def constant_classes(dtype):
    """``[('const', name, float32 c)]``: every class of the cast for a sample maximum M."""
    M = float(np.iinfo(dtype).max)
    vals = [('-0', -0.0), ('denormal', 1e-40), ('0.999', 0.999), ('-1e-3', -1e-3), ('-0.5', -0.5), ('-1', -1.0),
            ('-1.2M', -1.2 * M), ('M-0.5', M - 0.5), ('M', M), ('M+0.5', M + 0.5), ('M+1', M + 1.0),
            ('1.2M', 1.2 * M), ('2^31', 2.0 ** 31), ('2^32-256', 2.0 ** 32 - 256), ('2^32', 2.0 ** 32),
            ('3e38', 3e38), ('+inf', np.inf), ('-inf', -np.inf), ('nan', np.nan)]
    out = [('const', n, np.float32(v)) for n, v in vals]
    # the biases are what they are named after, exactly, in float32
    assert float(out[7][2]) == M - 0.5 and float(out[9][2]) == M + 0.5 and float(out[13][2]) == 2.0 ** 32 - 256
    assert np.signbit(out[0][2]) and 0 < float(out[1][2]) < np.finfo(np.float32).tiny
    return out


SMALL_K_CONSTANTS = ('-0', '-0.5', '-1', 'M', 'M+0.5', 'M+1', '2^32-256', '2^32', '+inf', '-inf', 'nan')


def classes(dtype, ndim):
    """The class cycle: all 19 constants, both saturating and three crossing channels for volumes
    (K = 19); for images (K = 5) the constants at the edges of each cast plus two crossing channels."""
    const = constant_classes(dtype)
    if ndim == 3:
        cross = [('cross', -0.5), ('cross', 0.0), ('cross', 0.5)]
    else:
        const = [c for c in const if c[1] in SMALL_K_CONSTANTS]
        cross = [('cross', -0.5), ('cross', 0.5)]
    # spread the data-dependent channels through the cycle: a set then holds them at distant channels
    cyc = list(const)
    extra = [('sat', -1.2), ('sat', 1.2)] + cross
    step = len(const) // len(extra)
    for i, c in enumerate(extra):
        cyc.insert(i * (step + 1), c)
    return cyc


class WeightSet:
    """``w [N, K]``, ``b [K]`` float32 and the class of each channel."""

    def __init__(self, w, b, cls, rotation):
        self.w, self.b, self.cls, self.rotation = w, b, cls, rotation

    def channels(self, kind):
        return [k for k, c in enumerate(self.cls) if c[0] == kind]


def noisy_mean_columns(n, k, seed=43):
    """_clamp_weights' columns (tests/test_gpu_guard.py), each scaled to sum to 1 so a saturating
    channel's distance from the range does not hang on the draw."""
    rng = np.random.default_rng(seed)
    w = (1.0 / n) * (1.0 + 0.3 * rng.standard_normal((n, k)))
    return (w / w.sum(axis=0, keepdims=True)).astype(np.float32)


def weight_sets(dtype, p, ndim):
    """One WeightSet per rotation of the class cycle (u8 / u16 samples)."""
    n, K = (2 * p + 2) ** ndim, NPRED[ndim]
    M = float(np.iinfo(dtype).max)
    cols = noisy_mean_columns(n, K)
    cyc = classes(dtype, ndim)
    sets = []
    for r in range(len(cyc)):
        w, b, cls = np.zeros((n, K), np.float32), np.zeros(K, np.float32), []
        for k in range(K):
            c = cyc[(k + r) % len(cyc)]
            cls.append(c)
            if c[0] == 'const':
                b[k] = c[2]
            else:
                w[:, k] = cols[:, k]
                b[k] = np.float32(c[1] * M)
        sets.append(WeightSet(w, b, cls, r))
    return sets


WIDE_CONSTANTS = ('-2^31', '2^31', '2^32', '+inf', '-inf', 'nan')


def weight_sets_32(dtype, p, ndim):
    """int32 / uint32 samples: noisy-mean columns with biases spread over 1.2 times the range
    (+-1.2 * 2^31, or [-0.2, 1.2] * 2^32; rotation 0), then sets whose even channels are the constants at
    +-2^31, 2^32, +-inf and NaN (zero columns), as many sets as it takes to place each once."""
    n, K = (2 * p + 2) ** ndim, NPRED[ndim]
    cols = noisy_mean_columns(n, K, seed=47)
    lo, hi = (-1.2 * 2.0 ** 31, 1.2 * 2.0 ** 31) if np.dtype(dtype) == np.int32 else (-0.2 * 2.0 ** 32, 1.2 * 2.0 ** 32)
    spread = np.random.default_rng(48).permutation(np.linspace(lo, hi, K)).astype(np.float32)
    sets = [WeightSet(cols.copy(), spread.copy(), [('spread', float(v)) for v in spread], 0)]
    if np.dtype(dtype) == np.uint32:
        # a noisy mean of full-range uint32 data sits near 2^31: with the biases above only the upper end
        # saturates, so a second set moves them down by 2^31 and the *predictions* span [-0.2, 1.2] * 2^32
        low = (spread.astype(np.float64) - 2.0 ** 31).astype(np.float32)
        sets.append(WeightSet(cols.copy(), low, [('spread', float(v)) for v in low], 0))
    consts = dict(zip(WIDE_CONSTANTS, np.array([-2.0 ** 31, 2.0 ** 31, 2.0 ** 32, np.inf, -np.inf, np.nan], np.float32)))
    even = list(range(0, K, 2))
    for r in range(-(-len(WIDE_CONSTANTS) // len(even))):
        w, b, cls = cols.copy(), spread.copy(), [('spread', float(v)) for v in spread]
        for j, k in enumerate(even):
            name = WIDE_CONSTANTS[(j + r * len(even)) % len(WIDE_CONSTANTS)]
            w[:, k], b[k], cls[k] = 0, consts[name], ('const', name, consts[name])
        sets.append(WeightSet(w, b, cls, r + 1))
    return sets


def data(shape, dtype, seed=1):
    """Full-range noise; 32-bit samples also get the range ends, 0 and values just past 2^24 (where
    the sample -> float32 conversion of the features starts to round) planted."""
    info = np.iinfo(dtype)
    rng = np.random.default_rng(seed)
    x = rng.integers(info.min, int(info.max) + 1, size=shape, dtype=np.int64).astype(dtype)
    if info.bits == 32:
        flat = x.reshape(-1)
        plant = np.array([info.min, info.max, 0, 2 ** 24 + 1, 2 ** 24 + 3, info.max - 1], np.int64).astype(dtype)
        idx = rng.choice(flat.size, size=4 * len(plant), replace=False)
        flat[idx] = np.tile(plant, 4)
    return x


def window_and_features(highres, p, ndim):
    """(padded highres, dims, the padded lowres window a predictor is called on, its features)."""
    o = ons(ndim)
    padded, dims = o.pad_highres(highres)
    window = o.pad_neighborhood(o.lowres_from_highres(padded), p)
    return padded, dims, window, o.features_from_lowres(window, p)


def f64_and_scale(features, ws):
    """The float64 predictions ``[.., K, C]`` and the tolerance scale ``sum |f||w| + |b|`` of finite
    channels (channels with a non-finite bias get an infinite scale: no claim rests on their margin)."""
    nd = features.ndim - 2
    f = np.moveaxis(features.astype(np.float64), nd, -1)
    w64 = ws.w.astype(np.float64)
    b64 = ws.b.astype(np.float64)
    with np.errstate(invalid='ignore'):
        v = np.moveaxis(np.tensordot(f, w64, axes=([-1], [0])), -1, nd) + b64.reshape(-1, 1)
        scale = np.moveaxis(np.tensordot(np.abs(f), np.abs(w64), axes=([-1], [0])), -1, nd) + np.abs(b64).reshape(-1, 1)
    return v, scale


def chain(features, ws):
    """The float32 values of arith='f32' (the oracle's k-ordered fma chain), ``[.., K, C]``."""
    with np.errstate(invalid='ignore'):  # inf - inf inside TwoSum on an infinite bias: the result is not used
        return OP.linear_fma_chain(features, ws.w, ws.b)


def expected_cells(features, ws, dtype, arith):
    """``(cells, decided)``, both ``[.., K, C]``: the cells every path must give and where that claim
    holds.  arith='f32': the cast of the oracle's chain, decided everywhere.  arith='bf16x2': the
    constants' casts; 0 / max on saturating channels, decided where the float64 value clears the
    range by MARGIN * scale (test_linear_cast_spec.py: that is everywhere); crossing channels
    undecided (filled with the f32 cells, which nothing may rely on)."""
    nd = features.ndim - 2
    if arith == 'f32':
        cells = cast_from_f32(chain(features, ws), dtype)
        return cells, np.ones(cells.shape, bool)
    assert arith == 'bf16x2'
    M = np.iinfo(dtype).max
    v, scale = f64_and_scale(features, ws)
    cells = np.zeros(v.shape, dtype)
    decided = np.zeros(v.shape, bool)
    for k, c in enumerate(ws.cls):
        ix = (slice(None),) * nd + (k,)
        if c[0] == 'const':
            cells[ix] = cast_from_f32(c[2], dtype)
            decided[ix] = True
        elif c[0] == 'sat':
            below, above = v[ix] <= -MARGIN * scale[ix], v[ix] >= M + MARGIN * scale[ix]
            cells[ix] = np.where(above, M, 0)
            decided[ix] = below | above
        else:
            cells[ix] = cast_from_f32(v[ix].astype(np.float32), dtype)
    return cells, decided


def expected_maps(cells, decided, ndim, dims):
    """The cells and the mask pushed through the aggregation: ``(maps, decided maps)``, trimmed; a
    map position is decided iff every cell its aggregation takes is."""
    o = ons(ndim)
    maps = o.trim_maps(o.maps_from_predictions(cells), dims)
    open_ = o.trim_maps(o.maps_from_predictions((~decided).astype(np.float32)), dims)
    return maps, tuple(m == 0 for m in open_)


# the channels each map aggregates (maps_from_predictions: L R | U D | F B | C | z0..3 | y0..3 | x0..3)
MAP_CHANNELS = {3: ((0, 1), (2, 3), (4, 5), (6,), (7, 8, 9, 10), (11, 12, 13, 14), (15, 16, 17, 18)),
                2: ((0, 1), (2, 3), (4,))}


def gt_maps(padded, ndim, dims):
    o = ons(ndim)
    return o.trim_maps(o.maps_from_highres(padded), dims)


def recover_predictions(gt, residuals):
    """The prediction maps a modular coder (uint8 / uint16 / uint32) used: ``(gt - residual) mod 2^bits``."""
    out = []
    for g, r in zip(gt, residuals):
        g, r = np.asarray(g), np.asarray(r)
        bits = g.dtype.itemsize * 8
        out.append(((g.astype(np.int64) - r.astype(np.int64)) % (1 << bits)).astype(g.dtype))
    return out


def mismatches(got_maps, want_maps, decided_maps, ws, limit=3):
    """``['map i at index: got g, want w; channel classes ...']`` for decided positions that differ."""
    lines = []
    by_map = MAP_CHANNELS[3 if len(ws.cls) == 19 else 2]
    for i, (g, w, d) in enumerate(zip(got_maps, want_maps, decided_maps)):
        bad = np.argwhere((np.asarray(g) != w) & d)
        for ix in bad[:limit]:
            ix = tuple(int(v) for v in ix)
            lines.append(f'rotation {ws.rotation} map {i} at {ix}: got {np.asarray(g)[ix]}, want {w[ix]} '
                         f'({len(bad)} in this map); channel classes {[(k, *ws.cls[k][:2]) for k in by_map[i]]}')
    return lines


def coders(ns, dtype):
    """(encode_fn, decode_fn) of a namespace (oracle or product) for the sample dtype."""
    name = {np.dtype(np.uint8): 'uint8', np.dtype(np.uint16): 'uint16', np.dtype(np.int32): 'raw',
            np.dtype(np.uint32): 'uint32'}[np.dtype(dtype)]
    return getattr(ns, 'encode_values_' + name), getattr(ns, 'decode_values_' + name)


def split_chunk(shape, ndim):
    """A chunk that splits the first axis it can (into two windows, or a few on a short axis) and
    leaves the others whole.  A chunk has at least 4 nodes, so a volume with fewer than 5 lowres nodes
    on every axis cannot be split: it runs as one window."""
    L = [(s + (s + 1) % 2 + 1) // 2 for s in shape[1:1 + ndim]]
    chunk, split = [], False
    for ext in L:
        if not split and ext >= 5:
            chunk.append(ext - 1)
            split = True
        else:
            chunk.append(max(ext, 4))
    return tuple(chunk)
