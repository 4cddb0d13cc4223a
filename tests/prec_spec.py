"""The relative-error float32 quantiser in numpy: the rule every kernel, ``kom.quant``'s relative
mode and the version-6 container are tested against.

The caller states ``rel_error``.  With ``mant, ex = frexp(rel_error)`` the quantiser keeps the top
``m = -ex`` mantissa bits of every float32, rounded to nearest even, and drops the low ``t = 23 - m``.
The bound kept is ``eps_rel = 2**-(m + 1)``: ``rel_error / 2 < eps_rel <= rel_error``; ``0 <= m <= 22``,
that is ``2**-23 <= rel_error < 1``.  For a float32 of bits ``u``, ``s = u >> 31``, ``a = u & 0x7fffffff``,
in 32-bit unsigned arithmetic:

    k = (a + 2**(t-1) - 1 + ((a >> t) & 1)) >> t
    x is an exception  iff  a >= 0x7f800000  or  (k << t) >= 0x7f800000  or  k > QMAX
    n = -k if s else k                                       (-0.0 gives 0)

The magnitude bits of a float32 are monotone in its magnitude, so ``n`` is a monotone integer image of
``x``.  Decoding is total: ``mag = |n|`` as uint32 (the type's minimum gives 2**15 or 2**31) and the
bits are ``((mag << t) & 0x7fffffff) | (0x80000000 if n < 0 else 0)``.  An exception is kept as its 32
raw bits; ENCODE writes it as the type's minimum, which no legal ``n`` takes (``|n| <= 255 * 2**m - 1``).
For every non-exception ``|r - x| <= eps_rel * max(|x|, 2**-126)``, and quantising ``r`` gives ``n`` again.
"""

import math

import numpy as np

M_MIN, M_MAX = 0, 22
QMAX = {np.dtype(np.int16): 32767, np.dtype(np.int32): 2 ** 31 - 1}
INF_BITS = 0x7f800000
# the mantissa widths the guarantee is checked at on random bit patterns
BITS = (0, 1, 7, 10, 15, 22)
# the largest m at which every n fits int16 (255 * 2**7 - 1 = 32639)
M_ALWAYS_I16 = 7


def mantissa_bits(rel_error):
    """``m``, the mantissa bits kept under ``rel_error``; ValueError for a bound that is no finite number
    in ``[2**-23, 1)``."""
    if isinstance(rel_error, (bool, str, bytes)) or not isinstance(rel_error, (int, float, np.integer, np.floating)):
        raise ValueError(f'rel_error must be a number in [2**-23, 1), got {rel_error!r}')
    try:
        a = float(rel_error)
    except OverflowError:
        a = math.inf
    if not math.isfinite(a) or a <= 0:
        raise ValueError(f'rel_error must be a number in [2**-23, 1), got {rel_error!r}')
    m = -math.frexp(a)[1]
    if not M_MIN <= m <= M_MAX:
        raise ValueError(f'rel_error {rel_error!r} is outside [2**-23, 1)')
    return m


def effective_rel(rel_error):
    """The relative bound the quantiser keeps: ``2**-(m + 1)``."""
    return math.ldexp(1.0, -(mantissa_bits(rel_error) + 1))


def sentinel(dtype):
    return np.iinfo(dtype).min


def _bits(x):
    x = np.ascontiguousarray(x)
    assert x.dtype == np.float32
    return x.view(np.uint32)


def quantise_as(x, m, dtype):
    """``(n as ``dtype`` with 0 at the exceptions, boolean exception mask)`` of float32 ``x``."""
    assert M_MIN <= m <= M_MAX
    t = np.uint32(23 - m)
    u = _bits(x)
    a = u & np.uint32(0x7fffffff)
    k = (a + np.uint32((1 << (23 - m - 1)) - 1) + ((a >> t) & np.uint32(1))) >> t
    exc = (a >= np.uint32(INF_BITS)) | ((k << t) >= np.uint32(INF_BITS)) | (k > np.uint32(QMAX[np.dtype(dtype)]))
    n = np.where(u >> np.uint32(31), -k.astype(np.int64), k.astype(np.int64))
    return np.where(exc, 0, n).astype(dtype), exc


def encode_bits(x, m, dtype):
    """What ``kmp_code`` ENCODE writes: ``n``, an exception as the type's minimum."""
    n, exc = quantise_as(x, m, dtype)
    n[exc] = sentinel(dtype)
    return n


def dequant(n, m):
    """What ``kmp_code`` DECODE writes for every int16 / int32 element, the type's minimum included."""
    n = np.asarray(n)
    assert n.dtype in (np.dtype(np.int16), np.dtype(np.int32)) and M_MIN <= m <= M_MAX
    mag = np.abs(n.astype(np.int64)).astype(np.uint32)  # 2**15 or 2**31 for the minimum
    bits = ((mag << np.uint32(23 - m)) & np.uint32(0x7fffffff)) | np.where(n < 0, np.uint32(0x80000000), np.uint32(0))
    return bits.astype(np.uint32).view(np.float32)


def quantise(x, m):
    """``(n, exceptions)``: int16 iff every non-exception fits it, else int32; ``exceptions`` is None
    or ``(flat C-order indices int64 ascending, raw bits uint32)``."""
    x = np.asarray(x)
    n, exc = quantise_as(x, m, np.int32)
    if np.abs(n.astype(np.int64)).max(initial=0) <= QMAX[np.dtype(np.int16)]:
        n16, exc16 = quantise_as(x, m, np.int16)
        assert np.array_equal(exc, exc16) and np.array_equal(n, n16)  # the same exception set under both types
        n = n16
    else:
        assert m > M_ALWAYS_I16
    idx = np.flatnonzero(exc.reshape(-1)).astype(np.int64)
    if idx.size == 0:
        return n, None
    return n, (idx, _bits(x).reshape(-1)[idx].copy())


def restore(n, m, exceptions):
    out = dequant(n, m).reshape(np.shape(n))
    if exceptions is not None:
        idx, bits = exceptions
        out.reshape(-1).view(np.uint32)[idx] = bits
    return out


def rel_errors(x, r):
    """``|r - x| / max(|x|, 2**-126)`` in float64, elementwise (finite inputs)."""
    xd, rd = np.asarray(x, np.float64), np.asarray(r, np.float64)
    return np.abs(rd - xd) / np.maximum(np.abs(xd), math.ldexp(1.0, -126))


# ---------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------

def _round_half_even(a, t):
    """``a / 2**t`` rounded to nearest, ties to even, in Python integers: the rule said another way."""
    q, r = divmod(a, 1 << t)
    half = 1 << (t - 1)
    return q + 1 if r > half or (r == half and q & 1) else q


def known_answers(m, dtype):
    """``(x float32, n expected, exception expected)`` around the rule's edges at ``m`` kept bits; the
    expectations come from integer division in Python, not from the shifts of ``quantise_as``."""
    t, qmax = 23 - m, QMAX[np.dtype(dtype)]
    half = 1 << (t - 1)
    one = 0x3f800000
    ktop = 255 * (1 << m) - 1  # the largest k whose restored value is finite
    mags = [
        0, 1, 0x007fffff, 0x00800000,                    # 0, the smallest and largest subnormal, the smallest normal
        one, one + half, one + (1 << t) + half,          # 1.0; ties: the even neighbour is below, then above
        one + half - 1, one + half + 1,                  # either side of a tie
        one | 0x007fffff, 0x42ffffff,                    # a mantissa of all ones: carries into the exponent
        (ktop << t) + half - 1, (ktop << t) + half,      # the largest that stays finite, the first that rounds to infinity
        0x7f7fffff, INF_BITS,                            # FLT_MAX, infinity
        0x7f800001, 0x7fc00000, 0x7fc12345, 0x7fffffff,  # NaNs with payloads
        half, half + 1, 3 * half,                        # subnormal ties: 0.5 -> 0, just above -> 1, 1.5 -> 2
    ]
    if qmax < ktop:  # the first k above QMAX and its neighbour below
        mags += [(qmax << t) + half - 1, (qmax << t) + half, (qmax + 1) << t, qmax << t]
    us, ns, es = [], [], []
    for a in mags:
        k = _round_half_even(a, t)
        exc = a >= INF_BITS or k > ktop or k > qmax
        for s in (0, 1):
            us.append(a | (s << 31))
            ns.append(0 if exc else (-k if s else k))
            es.append(exc)
    return np.array(us, np.uint32).view(np.float32), np.array(ns, np.int64), np.array(es, bool)


def random_bits(n, seed=0):
    """``n`` float32 values of uniformly random bit patterns (NaNs, infinities, subnormals included)."""
    return np.random.default_rng(seed).integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32).view(np.float32)


def decades_field(shape=(1, 40, 48, 56, 1), seed=0, noise=0.05):
    """A positive float32 field that spans about four decades (a smooth exponent) with multiplicative
    noise of relative size ``noise``: the field the size figures are quoted on."""
    import signed_spec
    rng = np.random.default_rng(seed)
    x = np.empty(shape, np.float64)
    for b in range(shape[0]):
        s = signed_spec.smooth_field(shape[1:-1], seed + b).astype(np.float64)
        s = (s - s.min()) / max(float(s.max() - s.min()), 1e-30)  # 0 .. 1
        x[b, ..., 0] = 10.0 ** (4.0 * s) * (1.0 + noise * rng.standard_normal(shape[1:-1]))
    return np.abs(x).astype(np.float32)
