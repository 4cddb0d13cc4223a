"""The error-bounded float32 quantiser in numpy: the rule every kernel, ``kom.quant`` and the
version-5 container are tested against.

The caller states ``abs_error``.  The step is the power of two ``2**e`` with ``m, e = frexp(abs_error)``
and the effective bound is ``eps = 2**(e - 1)``: ``abs_error / 2 < eps <= abs_error`` (a power-of-two
``abs_error`` is kept as it is).  For a float32 ``x`` and an integer type of largest value ``QMAX``, all
arithmetic in float64:

    n = rint(double(x) * 2**-e)              ties to even
    r = float32(double(n) * 2**e)
    x is an exception  iff  x is not finite, |n| > QMAX, r is not finite or |double(r) - double(x)| > eps

Both products are exact (a power of two times a float32 or an integer below 2**31 fits a float64), so
the only rounding is the conversion to float32 and the rule gives the same bits everywhere.  A
non-exception restores to ``r`` (``-0.0`` as ``+0.0``), an exception is kept as its 32 raw bits.
"""

import math

import numpy as np

import signed_spec

E_MIN, E_MAX = -126, 127
QMAX = {np.dtype(np.int16): 32767, np.dtype(np.int32): 2 ** 31 - 1}
# the exponents the bound is checked at on random bit patterns
EXPONENTS = (-126, -60, -10, 0, 20, 100, 127)


def exponent(abs_error):
    """``e`` of the step ``2**e``; ValueError for a bound that is no positive finite number or whose
    exponent is outside ``[E_MIN, E_MAX]``."""
    if isinstance(abs_error, (bool, str, bytes)) or not isinstance(abs_error, (int, float, np.integer, np.floating)):
        raise ValueError(f'abs_error must be a positive finite number, got {abs_error!r}')
    a = float(abs_error)
    if not math.isfinite(a) or a <= 0:
        raise ValueError(f'abs_error must be a positive finite number, got {abs_error!r}')
    e = math.frexp(a)[1]
    if not E_MIN <= e <= E_MAX:
        raise ValueError(f'abs_error {abs_error!r}: step exponent {e} outside [{E_MIN}, {E_MAX}]')
    return e


def effective(abs_error):
    """The bound the quantiser keeps: ``2**(e - 1)``."""
    return math.ldexp(1.0, exponent(abs_error) - 1)


def quantise_as(x, e, dtype):
    """``(n as ``dtype`` with 0 at the exceptions, boolean exception mask)`` of float32 ``x``."""
    x = np.asarray(x)
    assert x.dtype == np.float32 and E_MIN <= e <= E_MAX
    qmax = QMAX[np.dtype(dtype)]
    with np.errstate(all='ignore'):
        xd = x.astype(np.float64)
        n = np.rint(xd * math.ldexp(1.0, -e))
        r = (n * math.ldexp(1.0, e)).astype(np.float32)
        ok = np.isfinite(xd) & (np.abs(n) <= qmax) & np.isfinite(r) & \
            (np.abs(r.astype(np.float64) - xd) <= math.ldexp(1.0, e - 1))
    return np.where(ok, n, 0.0).astype(dtype), ~ok


def sentinel(dtype):
    return np.iinfo(dtype).min


def encode_bits(x, e, dtype):
    """What ``kmp_code`` ENCODE writes: ``n``, an exception as the type's minimum."""
    n, exc = quantise_as(x, e, dtype)
    n[exc] = sentinel(dtype)
    return n


def dequant(n, e):
    """What ``kmp_code`` DECODE writes for every element: ``float32(double(n) * 2**e)``."""
    with np.errstate(all='ignore'):
        return (np.asarray(n).astype(np.float64) * math.ldexp(1.0, e)).astype(np.float32)


def quantise(x, e):
    """``(n, exceptions)``: int16 iff every non-exception fits it, else int32; ``exceptions`` is None
    or ``(flat C-order indices int64 ascending, raw bits uint32)``."""
    x = np.asarray(x)
    n, exc = quantise_as(x, e, np.int32)
    if np.abs(n.astype(np.int64)).max(initial=0) <= QMAX[np.dtype(np.int16)]:
        n16, exc16 = quantise_as(x, e, np.int16)
        assert np.array_equal(exc, exc16) and np.array_equal(n, n16)  # the same exception set under both types
        n = n16
    idx = np.flatnonzero(exc.reshape(-1)).astype(np.int64)
    if idx.size == 0:
        return n, None
    return n, (idx, np.ascontiguousarray(x).reshape(-1).view(np.uint32)[idx].copy())


def restore(n, e, exceptions):
    out = dequant(n, e)
    if exceptions is not None:
        idx, bits = exceptions
        out.reshape(-1).view(np.uint32)[idx] = bits
    return out


def gaps_from_indices(idx):
    """``(low words, high words)`` of the gaps between consecutive sorted indices (the first gap is the
    first index), as the container stores them."""
    idx = np.asarray(idx, np.int64)
    g = np.diff(idx, prepend=np.int64(0)).astype(np.uint64)
    return (g & np.uint64(0xffffffff)).astype(np.uint32), (g >> np.uint64(32)).astype(np.uint32)


def indices_from_gaps(lo, hi):
    return np.cumsum(lo.astype(np.int64) | (hi.astype(np.int64) << 32)).astype(np.int64)


def level_exceptions(exceptions, shape, ndim, k):
    """The exceptions of pyramid level ``k`` of an array of ``shape = (B, spatial..., C...)``: those
    whose spatial coordinates are all multiples of ``2**k``, indexed in the strided array."""
    idx, bits = exceptions
    coords = list(np.unravel_index(idx, shape))
    keep = np.ones(idx.shape, bool)
    for a in range(1, 1 + ndim):
        keep &= coords[a] % (2 ** k) == 0
        coords[a] = coords[a] // (2 ** k)
    lshape = tuple(-(-s // 2 ** k) if 1 <= a <= ndim else s for a, s in enumerate(shape))
    return np.ravel_multi_index([c[keep] for c in coords], lshape).astype(np.int64), bits[keep], lshape


# ---------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------

def known_answers(e, dtype):
    """``(x float32, n expected, exception expected)`` around the rule's edges at exponent ``e``."""
    step, qmax = math.ldexp(1.0, e), QMAX[np.dtype(dtype)]
    rows = [(0.5 * step, 0, False), (1.5 * step, 2, False), (2.5 * step, 2, False), (-0.5 * step, 0, False),
            (-1.5 * step, -2, False), (0.0, 0, False), (-0.0, 0, False), (step, 1, False), (-step, -1, False),
            (math.nan, 0, True), (math.inf, 0, True), (-math.inf, 0, True)]
    # the largest n accepted (float32 holds 2**31 - 128 exactly, not 2**31 - 1) and the first refused
    top = qmax if qmax < 2 ** 24 else 2 ** 31 - 128
    for s in (1.0, -1.0):
        rows += [(s * top * step, int(s * top), False), (s * (qmax + 1) * step, 0, True)]
    fmax = float(np.finfo(np.float32).max)
    # only rows float32 holds exactly and whose restored value is finite (at e = 127: |n| <= 1)
    rows = [r for r in rows if not math.isfinite(r[0]) or
            (abs(r[0]) <= fmax and float(np.float32(r[0])) == r[0] and (r[2] or abs(r[1]) * step <= fmax))]
    xs = np.array([r[0] for r in rows], np.float32)
    return xs, np.array([r[1] for r in rows], np.int64), np.array([r[2] for r in rows], bool)


def random_bits(n, seed=0):
    """``n`` float32 values of uniformly random bit patterns (NaNs, infinities, subnormals included)."""
    return np.random.default_rng(seed).integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32).view(np.float32)


def spec_field():
    """The 40 x 48 x 56 smooth-plus-noise float32 field the size figures are quoted on."""
    import near_spec
    f = near_spec.noisy_field((1, 40, 48, 56, 1), np.uint16, seed=0)
    u = np.random.default_rng(7).uniform(-.5, .5, size=f.shape)
    return ((f.astype(np.float64) - 2000.0) / 300.0 + u / 300.0).astype(np.float32)


def pyramid_bits(n, ndim, padding, levels):
    """Rice bits per sample (oracle.rice) of int16 ``n`` as a ``levels``-deep MeanPredictor pyramid."""
    fn = signed_spec.mean_fn(padding, ndim)
    arrays, x = [], n
    for _ in range(levels):
        x, maps, _ = signed_spec.encode(x, fn, ndim, padding)
        arrays.extend(maps)
    arrays.append(x)
    return signed_spec.rice_bits_per_sample(arrays) * sum(a.size for a in arrays) / n.size
