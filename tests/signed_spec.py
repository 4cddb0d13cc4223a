"""Signed samples (int8 / int16), as a specification: the sign map, the codec on signed data stated as
the oracle's codec on mapped data, the stand-alone coders, and the data every signed test runs on.
Shared by test_signed_spec.py (the conditions, from the oracle alone), the golden fixtures
(tests/golden/make_golden_signed.py) and the test_gpu_signed*.py files (the kernels).  Pure numpy +
oracle; knows nothing of the product.

One rule.  ``M(x) = x ^ signbit`` maps a signed type onto the unsigned type of its width and keeps
the order (it is ``x + 2^(W-1)``).  A built-in predictor sees ``M(samples)`` and runs the unsigned
arithmetic; the residual is ``(M(gt) - P) mod 2^W`` in the unsigned type; every sample-domain array
a caller passes or gets (highres, lowres, predictions) is in the signed type, ``M^-1`` of the
mapped one.  So: codec(x) = codec_unsigned(M(x)), with lowres and highres mapped back."""

import numpy as np

import oracle
from oracle import predictors as OP
from oracle import rice as ORice

SIGNED = (np.int8, np.int16)
UNSIGNED = {np.dtype(np.int8): np.dtype(np.uint8), np.dtype(np.int16): np.dtype(np.uint16)}


def ons(ndim):
    return oracle.volume if ndim == 3 else oracle.image


def unsigned_of(dtype):
    return UNSIGNED[np.dtype(dtype)]


def signbit(dtype):
    return 1 << (np.dtype(dtype).itemsize * 8 - 1)


def M(x):
    """Signed array -> the unsigned array of the same width, order preserved: ``x ^ signbit``."""
    x = np.ascontiguousarray(x)
    u = unsigned_of(x.dtype)
    return x.view(u) ^ u.type(signbit(u))


def Minv(u):
    """The inverse of :func:`M`: unsigned array -> the signed array of the same width."""
    u = np.ascontiguousarray(u)
    s = {v: k for k, v in UNSIGNED.items()}[u.dtype]
    return (u ^ u.dtype.type(signbit(u.dtype))).view(s)


def unsigned_coders(dtype):
    u = unsigned_of(dtype)
    c = oracle.common
    return (c.encode_values_uint8, c.decode_values_uint8) if u == np.uint8 else (c.encode_values_uint16,
                                                                                 c.decode_values_uint16)


def encode_values(pred, gt):
    """``encode_values_int8 / int16``: ``(gt - pred) mod 2^W`` on the signed values, in the unsigned
    type.  (No map: it cancels in the difference.)"""
    gt = np.asarray(gt)
    W = gt.dtype.itemsize * 8
    d = (gt.astype(np.int64) - np.asarray(pred).astype(np.int64)) % (1 << W)
    return d.astype(unsigned_of(gt.dtype))


def decode_values(pred, enc, dtype):
    """``decode_values_int8 / int16``: the signed value ``(pred + enc) mod 2^W`` reads as."""
    W = np.dtype(dtype).itemsize * 8
    v = (np.asarray(pred).astype(np.int64) + np.asarray(enc).astype(np.int64)) % (1 << W)
    return v.astype(unsigned_of(dtype)).view(dtype)


def mean_fn(padding, ndim):
    return OP.mean_predictions_fn(padding, ndim)


def linear_fn(padding, weights, bias, ndim):
    return OP.linear_predictions_fn(padding, weights, bias, ndim)


def encode(x, predictions_fn, ndim, padding):
    """``(lowres signed, maps unsigned, dims)`` of signed highres ``x`` under an oracle predictions_fn
    (mean_fn / linear_fn), which sees ``M(x)``."""
    enc, _ = unsigned_coders(x.dtype)
    lo, (maps, dims) = ons(ndim).encode(predictions_fn, enc, M(x), padding=padding)
    return Minv(lo), tuple(maps), tuple(int(d) for d in dims)


def decode(lowres, maps, dims, predictions_fn, ndim, padding):
    _, dec = unsigned_coders(lowres.dtype)
    return Minv(ons(ndim).decode(predictions_fn, dec, M(lowres), (tuple(maps), tuple(dims)), padding=padding))


def predictions(window, predictions_fn):
    """The prediction maps a built-in predictor returns for a signed padded-lowres window:
    ``M^-1`` of the unsigned predictor's maps of ``M(window)``."""
    return tuple(Minv(np.asarray(m)) for m in predictions_fn(M(window)))


# ---------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------

def extremes(dtype):
    info = np.iinfo(dtype)
    return np.array([info.min, -1, 0, 1, info.max], dtype)


def smooth_field(shape, seed=0):
    """A smooth float field in about [-1, 1] on the spatial ``shape``, offset so that about 60 % of it
    is negative."""
    rng = np.random.default_rng(seed)
    axes = np.meshgrid(*[np.linspace(0.0, 1.0, s) for s in shape], indexing='ij')
    f = np.zeros(shape)
    for _ in range(4):
        k = rng.uniform(0.5, 2.5, size=len(shape))
        ph = rng.uniform(0, 2 * np.pi)
        f += np.sin(2 * np.pi * sum(ki * a for ki, a in zip(k, axes)) + ph)
    f /= np.abs(f).max()
    return f - np.quantile(f, 0.6)


def zero_crossing(shape, dtype=np.int16, seed=0, scale=300.0, noise=20.0):
    """``round(scale * f + noise * n)`` on ``shape = (B, spatial..., C)``: smooth, crossing zero, with
    about 60 % of the samples negative.  int8 data scales to its range (scale 60, noise 4)."""
    if np.dtype(dtype) == np.int8 and scale == 300.0:
        scale, noise = 60.0, 4.0
    rng = np.random.default_rng(seed + 1)
    sp = shape[1:-1]
    out = np.empty(shape, np.float64)
    for b in range(shape[0]):
        for c in range(shape[-1]):
            out[b, ..., c] = scale * smooth_field(sp, seed + 7 * b + c) + noise * rng.standard_normal(sp)
    info = np.iinfo(dtype)
    return np.clip(np.round(out), info.min, info.max).astype(dtype)


def uniform(shape, dtype, seed=0):
    info = np.iinfo(dtype)
    return np.random.default_rng(seed).integers(info.min, int(info.max) + 1, size=shape, dtype=np.int64).astype(dtype)


def data(shape, dtype, seed=0):
    """The array a signed codec test runs on: batch entry 0 the zero-crossing field, the others
    uniform noise over the whole range (a one-entry batch: the field in its first half, noise in the
    second), with the extremes -2^(W-1), -1, 0, 1, 2^(W-1)-1 planted at both ends of every entry."""
    x = uniform(shape, dtype, seed)
    zc = zero_crossing((1,) + tuple(shape[1:]), dtype, seed)[0]
    if shape[0] > 1:
        x[0] = zc
    else:
        h = shape[1] // 2
        x[0, :h] = zc[:h]
    ex = extremes(dtype)
    flat = x.reshape(shape[0], -1)
    flat[:, :ex.size] = ex
    flat[:, -ex.size:] = ex[::-1]
    return x


def rice_bits_per_sample(arrays):
    """Rice payload + side information (oracle.rice) of the arrays, in bits per sample."""
    bits = n = 0
    for a in arrays:
        params, bw = ORice.plan(np.asarray(a).reshape(-1))
        bits += 32 * int(bw.astype(np.int64).sum()) + 16 * params.size
        n += a.size
    return bits / n


def clamp_weights(n, k, seed=43):
    """Noisy-mean LinearPredictor weights (each column sums to about 1) and a small bias: predictions
    stay near the data, on both sides of the mapped range's edges for full-range noise."""
    rng = np.random.default_rng(seed)
    w = ((1.0 / n) * (1.0 + 0.3 * rng.standard_normal((n, k)))).astype(np.float32)
    b = rng.uniform(-3.0, 3.0, size=k).astype(np.float32)
    return w, b
