"""Near-lossless coding (``max_error``), as a specification: the quantising coder, one level of the
codec with it, the closed loop over the pyramid, and the data the near tests run on.  Shared by
test_near_spec.py (the rule's own consequences, from the oracle alone) and the test_gpu_near*.py
files (the kernels, the Python layers and the files).  Pure numpy + oracle; knows nothing of the
product.

The rule.  Samples are uint8 / uint16 / int8 / int16, W bits wide, MAX = 2^W - 1; signed types work on
``M(x)`` (signed_spec).  ``1 <= delta <= 2^(W-1) - 1`` and ``step = 2 delta + 1``.  For a prediction
``P`` (an integer clamped to [0, MAX]; a float32 prediction is truncated first, NaN -> 0, and clamped
to the sample type's own range) and a sample ``x``:

    e = x - P,   q = sign(e) * ((|e| + delta) // step),   R = clamp(P + q * step, 0, MAX)

``q`` is stored as W-bit two's complement in the unsigned map dtype; ``|R - x| <= delta``.
``delta = 0`` is not a quantiser: it names the modular coder of the dtype."""

import numpy as np

import oracle
from oracle import predictors as OP

from signed_spec import M, Minv, ons, rice_bits_per_sample, smooth_field, unsigned_of  # noqa: F401

DTYPES = (np.uint8, np.uint16, np.int8, np.int16)


def width(dtype):
    return np.dtype(dtype).itemsize * 8


def max_delta(dtype):
    return (1 << (width(dtype) - 1)) - 1


def is_signed(dtype):
    return np.dtype(dtype).kind == 'i'


def map_dtype(dtype):
    return np.dtype(f'uint{width(dtype)}')


def check(dtype, delta):
    if np.dtype(dtype) not in [np.dtype(d) for d in DTYPES]:
        raise TypeError(f'no near-lossless coder for {np.dtype(dtype)}')
    if isinstance(delta, bool) or not isinstance(delta, (int, np.integer)) or not 1 <= delta <= max_delta(dtype):
        raise ValueError(f'max_error {delta!r} outside [1, {max_delta(dtype)}]')


def mapped(a):
    """The samples as numbers in [0, MAX] (int64): ``a`` itself, or ``M(a)`` for a signed array."""
    a = np.asarray(a)
    return (M(a) if is_signed(a.dtype) else a).astype(np.int64)


def unmapped(v, dtype):
    """The inverse of :func:`mapped`: numbers in [0, MAX] -> the array of ``dtype``."""
    u = np.asarray(v).astype(map_dtype(dtype))
    return Minv(u) if is_signed(dtype) else u


def pred_int(pred, dtype):
    """The prediction as the rule's integer ``P`` in [0, MAX] (int64).  ``pred`` is an array of the
    sample dtype, or float32: truncated toward zero, NaN -> 0, clamped to the sample type's range."""
    pred = np.asarray(pred)
    if pred.dtype == np.float32:
        info = np.iinfo(dtype)
        with np.errstate(invalid='ignore'):
            t = np.trunc(np.where(np.isnan(pred), np.float32(0), pred).astype(np.float64))
        t = np.clip(t, info.min, info.max).astype(np.int64)
        return t - info.min  # M on the numbers: x + 2^(W-1) for a signed type, x for an unsigned one
    if pred.dtype != np.dtype(dtype):
        raise TypeError(f'predictions must be {np.dtype(dtype)} or float32, got {pred.dtype}')
    return mapped(pred)


def quantise(P, x, delta):
    """``q`` (int64) of integer arrays ``P``, ``x`` in [0, MAX]."""
    e = np.asarray(x, np.int64) - np.asarray(P, np.int64)
    return np.sign(e) * ((np.abs(e) + delta) // (2 * delta + 1))


def reconstruct(P, q, delta, W):
    """``R`` (int64) and the unclamped ``P + q step``."""
    raw = np.asarray(P, np.int64) + np.asarray(q, np.int64) * (2 * delta + 1)
    return np.clip(raw, 0, (1 << W) - 1), raw


def encode_values(pred, gt, delta):
    """The near encoder: the map of ``q`` in the unsigned map dtype (W-bit two's complement)."""
    gt = np.asarray(gt)
    check(gt.dtype, delta)
    q = quantise(pred_int(pred, gt.dtype), mapped(gt), delta)
    return (q % (1 << width(gt.dtype))).astype(map_dtype(gt.dtype))


def signed_q(enc):
    """The stored map read back as the signed number ``q`` (int64)."""
    enc = np.asarray(enc)
    return enc.view(np.dtype(f'int{enc.dtype.itemsize * 8}')).astype(np.int64)


def decode_values(pred, enc, delta, dtype):
    """The near decoder: ``R`` in the sample dtype."""
    check(dtype, delta)
    R, _ = reconstruct(pred_int(pred, dtype), signed_q(enc), delta, width(dtype))
    return unmapped(R, dtype)


def coders(dtype, delta):
    """``(encode_fn, decode_fn)`` for the oracle's ``encode`` / ``decode`` on arrays of ``dtype``."""
    return (lambda pred, gt: encode_values(pred, gt, delta),
            lambda pred, enc: decode_values(pred, enc, delta, dtype))


# ---------------------------------------------------------------------------------------------------
# predictors (as the oracle's predictions_fn on *mapped* windows, lifted to the sample dtype)
# ---------------------------------------------------------------------------------------------------

def lifted(predictions_fn, dtype, as_f32=False):
    """A predictions_fn on windows of ``dtype``: a built-in predictor sees ``M(window)`` and its maps
    come back as ``M^-1`` (signed_spec); ``as_f32``: the maps as float32 numbers in the sample domain,
    the shape of a network's output."""
    def fn(window):
        window = np.asarray(window)
        maps = predictions_fn(M(window) if is_signed(dtype) else window)
        maps = [Minv(np.asarray(m)) if is_signed(dtype) else np.asarray(m) for m in maps]
        return tuple(m.astype(np.float32) for m in maps) if as_f32 else tuple(maps)
    return fn


def mean_fn(padding, ndim, dtype, as_f32=False):
    return lifted(OP.mean_predictions_fn(padding, ndim), dtype, as_f32)


def linear_fn(padding, weights, bias, ndim, dtype, as_f32=False):
    return lifted(OP.linear_predictions_fn(padding, weights, bias, ndim), dtype, as_f32)


def linear_weights(padding, ndim, seed=43):
    """Noisy-mean LinearPredictor weights (signed_spec.clamp_weights): predictions on both sides of
    the range's edges for full-range noise."""
    n, k = (2 * padding + 2) ** ndim, 19 if ndim == 3 else 5
    rng = np.random.default_rng(seed)
    w = ((1.0 / n) * (1.0 + 0.3 * rng.standard_normal((n, k)))).astype(np.float32)
    b = rng.uniform(-3.0, 3.0, size=k).astype(np.float32)
    return w, b


# ---------------------------------------------------------------------------------------------------
# one level, and the closed loop
# ---------------------------------------------------------------------------------------------------

def encode_level(h, predictions_fn, ndim, padding, delta):
    """``(lowres, maps, dims)`` of highres ``h``: the nodes exactly, ``q`` for every other cell."""
    enc, _ = coders(h.dtype, delta)
    lo, (maps, dims) = ons(ndim).encode(predictions_fn, enc, h, padding=padding)
    return np.ascontiguousarray(lo), tuple(np.ascontiguousarray(m) for m in maps), tuple(int(d) for d in dims)


def decode_level(lowres, maps, dims, predictions_fn, ndim, padding, delta):
    """The nodes unchanged and ``R`` elsewhere."""
    _, dec = coders(lowres.dtype, delta)
    return np.ascontiguousarray(ons(ndim).decode(predictions_fn, dec, lowres, (tuple(maps), tuple(dims)),
                                                 padding=padding))


def strided(x, ndim, k):
    s = 2 ** k
    return x[(slice(None), *[slice(None, None, s)] * ndim)]


def encode_pyramid(x, predictions_fn, ndim, padding, levels, delta):
    """The closed loop, coarsest level first: ``(lowres r_L, [(maps, dims), ...] finest first,
    [r_0, ..., r_L])``.  Level k's maps are the one-level maps of ``x_k`` with its nodes replaced by
    ``r_{k+1}``, and ``r_k`` is their decode."""
    xs = [np.ascontiguousarray(strided(x, ndim, k)) for k in range(levels + 1)]
    r = [None] * (levels + 1)
    r[levels] = xs[levels]
    enc = [None] * levels
    for k in reversed(range(levels)):
        h = xs[k].copy()
        strided(h, ndim, 1)[...] = r[k + 1]
        lo, maps, dims = encode_level(h, predictions_fn, ndim, padding, delta)
        assert np.array_equal(lo, r[k + 1])
        enc[k] = (maps, dims)
        r[k] = decode_level(lo, maps, dims, predictions_fn, ndim, padding, delta)
    return r[levels], enc, r


def decode_pyramid(lowres, encoded, predictions_fn, ndim, padding, delta):
    """The existing coarsest-first loop with the dequantising coder."""
    x = lowres
    for maps, dims in reversed(list(encoded)):
        x = decode_level(x, maps, dims, predictions_fn, ndim, padding, delta)
    return x


# ---------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------

def extremes(dtype):
    info = np.iinfo(dtype)
    mid = (int(info.min) + int(info.max)) // 2
    return np.array([info.min, info.min + 1, mid, mid + 1, info.max - 1, info.max], dtype)


def noise(shape, dtype, seed=0):
    """Full-range uniform noise with the extremes planted at both ends of every batch entry."""
    info = np.iinfo(dtype)
    x = np.random.default_rng(seed).integers(info.min, int(info.max) + 1, size=shape, dtype=np.int64).astype(dtype)
    ex = extremes(dtype)
    flat = x.reshape(shape[0], -1)
    flat[:, :ex.size] = ex
    flat[:, -ex.size:] = ex[::-1]
    return x


def noisy_field(shape, dtype=np.uint16, seed=0, base=2000.0, scale=300.0, sigma=20.0):
    """``round(base + scale * smooth + sigma * n)`` on ``shape = (B, spatial..., C)``: a smooth field
    under detector-like noise.  8-bit data scales to its range; signed data is centred on zero."""
    if width(dtype) == 8:
        base, scale, sigma = 120.0, 60.0, 4.0
    if is_signed(dtype):
        base = 0.0
    rng = np.random.default_rng(seed + 1)
    sp = shape[1:-1]
    out = np.empty(shape, np.float64)
    for b in range(shape[0]):
        for c in range(shape[-1]):
            out[b, ..., c] = base + scale * smooth_field(sp, seed + 7 * b + c) + sigma * rng.standard_normal(sp)
    info = np.iinfo(dtype)
    return np.clip(np.round(out), info.min, info.max).astype(dtype)


def rice_bits(encoded, lowres=None):
    """Rice bits per coded sample (payload + side information, oracle.rice) of a pyramid's maps,
    the coarsest lowres included when given."""
    arrays = [m for maps, _ in encoded for m in maps]
    if lowres is not None:
        arrays.append(lowres)
    return rice_bits_per_sample(arrays)


# the tables the coder tests run on
U8_DELTAS = (1, 2, 3, 7, 63, 127)
U16_DELTAS = (1, 2, 100, 255, 21845, 32767)


def u16_predictions(delta):
    step = 2 * delta + 1
    return np.array([0, 1, step - 1, step, 32767, 32768, 65534, 65535], np.int64)


def pair_table(dtype, delta):
    """``(pred, x)`` arrays of ``dtype``: every (P, x) pair for 8-bit samples, the boundary
    predictions of :func:`u16_predictions` against every x for 16-bit ones (in mapped numbers)."""
    W = width(dtype)
    xs = np.arange(1 << W, dtype=np.int64)
    ps = xs if W == 8 else u16_predictions(delta)
    P, X = np.meshgrid(ps, xs, indexing='ij')
    return unmapped(P.reshape(-1), dtype), unmapped(X.reshape(-1), dtype)


def f32_predictions(n, dtype, seed=5):
    """float32 predictions that exercise the cast: in-range fractions, values past both ends of the
    sample range, huge values, infinities and NaN."""
    info = np.iinfo(dtype)
    rng = np.random.default_rng(seed)
    v = rng.uniform(float(info.min) - 40.0, float(info.max) + 40.0, size=n).astype(np.float32)
    special = np.array([np.nan, np.inf, -np.inf, 3e9, -3e9, 1e20, -1e20, info.min - 0.5, info.max + 0.5, -0.75, 0.75,
                        float(info.min), float(info.max)], np.float32)
    v[:special.size] = special
    return v
