"""The error statistics of a restored array against its original, in numpy: the rule the comparing
kernels, ``kom.metrics`` and the containers' quality figures are tested against.

Inputs: two arrays of one dtype and one length -- float32, uint8, uint16, int8 or int16 -- ``x`` the
original and ``r`` the restored one.

* float32: element ``i`` is COMPARED iff ``x_i`` and ``r_i`` are both finite; otherwise it is a MISMATCH
  iff their 32-bit patterns differ (a NaN or an infinity restored bit for bit is neither).
* integer dtypes: every element is compared, there are no mismatches.

Over the compared elements, ``e_i = double(r_i) - double(x_i)`` (exact in float64), the RECORD is eight
64-bit words:

    0  count (u64)                   1  mismatch (u64)
    2  max |e_i| as f64 bits; 0.0 when count == 0
    3  sse = sum e_i^2: float32 input f64 bits, integer input u64 (exact)
    4, 5  min / max of the compared x_i as f64 bits, a zero as +0.0; +inf / -inf when count == 0
    6, 7  0

Derived on the host: ``mse = sse / count`` (0.0 when count == 0), ``rmse = sqrt(mse)``, ``value_range =
x_max - x_min`` (0.0 when count == 0), ``peak`` = the value range for float32 and ``2^W - 1`` for integer
samples unless the caller passes a positive finite one, ``psnr = inf`` if ``mse == 0`` else ``-inf`` if
``peak == 0`` else ``10 log10(peak^2 / mse)``, ``nrmse = rmse / peak`` (``inf`` when ``peak == 0`` and
``rmse > 0``, 0.0 when both are 0).

Every word is pinned bit for bit but the float32 ``sse``, which depends on the order of a float64 sum
of non-negative terms: any order stays within ``(n - 1) 2^-53`` relative of the exact sum to first
order, so a device's value is checked with :func:`sse_ok` -- ``|sse - fsum(e_i^2)| <= n 2^-52 fsum`` -- and
must be the same 64 bits on every call.
"""

import math

import numpy as np

DTYPES = (np.float32, np.uint8, np.uint16, np.int8, np.int16)
WORDS = 8


def _pair(x, r):
    x, r = np.ascontiguousarray(x).reshape(-1), np.ascontiguousarray(r).reshape(-1)
    assert x.dtype == r.dtype and x.dtype in [np.dtype(d) for d in DTYPES] and x.shape == r.shape
    return x, r


def squares(x, r):
    """``(compared mask, e_i^2 of the compared elements as float64 -- exact integers for integer input)``."""
    x, r = _pair(x, r)
    if x.dtype == np.float32:
        ok = np.isfinite(x) & np.isfinite(r)
        e = r[ok].astype(np.float64) - x[ok].astype(np.float64)
        return ok, e * e
    e = r.astype(np.int64) - x.astype(np.int64)
    return np.ones(x.shape, bool), (e * e).astype(np.float64)  # below 2^32: exact


def record(x, r):
    """``{'count', 'mismatch', 'max_abs', 'sse', 'x_min', 'x_max'}``: Python ints and floats; the float32
    ``sse`` is ``math.fsum`` of the squares (the correctly rounded sum), the integer one an exact int."""
    x, r = _pair(x, r)
    if x.dtype == np.float32:
        ok, sq = squares(x, r)
        mismatch = int(np.count_nonzero(~ok & (x.view(np.uint32) != r.view(np.uint32))))
        xs = x[ok].astype(np.float64)
        e = np.abs(r[ok].astype(np.float64) - xs)
        sse = math.fsum(sq.tolist())
    else:
        xs = x.astype(np.float64)
        d = r.astype(np.int64) - x.astype(np.int64)
        e = np.abs(d).astype(np.float64)
        mismatch, sse = 0, int((d * d).sum(dtype=np.uint64)) if d.size else 0
    count = int(xs.size)
    return {'count': count, 'mismatch': mismatch, 'max_abs': float(e.max()) if count else 0.0, 'sse': sse,
            'x_min': float(xs.min()) + 0.0 if count else math.inf,  # -0.0 + 0.0 is +0.0
            'x_max': float(xs.max()) + 0.0 if count else -math.inf}


def _f64_bits(v):
    return int(np.array([v], np.float64).view(np.uint64)[0])


def words(rec, is_float):
    """The record as its eight uint64 words."""
    sse = _f64_bits(rec['sse']) if is_float else int(rec['sse'])
    return np.array([rec['count'], rec['mismatch'], _f64_bits(rec['max_abs']), sse, _f64_bits(rec['x_min']),
                     _f64_bits(rec['x_max']), 0, 0], np.uint64)


def from_words(w, is_float):
    """The record of eight uint64 words."""
    w = np.ascontiguousarray(w, np.uint64)
    f = w.view(np.float64)
    return {'count': int(w[0]), 'mismatch': int(w[1]), 'max_abs': float(f[2]),
            'sse': float(f[3]) if is_float else int(w[3]), 'x_min': float(f[4]), 'x_max': float(f[5])}


def sse_ok(sse, n, exact):
    """The float32 rule's bound on a device's ``sse`` against ``exact = fsum(e_i^2)`` over ``n`` elements."""
    return abs(sse - exact) <= n * 2.0 ** -52 * exact


def fold(a, b):
    """The record of a concatenation from its parts' records (continue mode)."""
    return {'count': a['count'] + b['count'], 'mismatch': a['mismatch'] + b['mismatch'],
            'max_abs': max(a['max_abs'], b['max_abs']), 'sse': a['sse'] + b['sse'],
            'x_min': min(a['x_min'], b['x_min']), 'x_max': max(a['x_max'], b['x_max'])}


def default_peak(rec, dtype):
    dtype = np.dtype(dtype)
    if dtype == np.float32:
        return rec['x_max'] - rec['x_min'] if rec['count'] else 0.0
    return float(2 ** (8 * dtype.itemsize) - 1)


def derive(rec, dtype, peak=None):
    """The host arithmetic on a record: ``{'count', 'mismatch', 'max_abs_error', 'mse', 'rmse', 'psnr',
    'nrmse', 'value_range', 'peak'}``."""
    count = rec['count']
    mse = float(rec['sse']) / count if count else 0.0
    rmse = math.sqrt(mse)
    value_range = rec['x_max'] - rec['x_min'] if count else 0.0
    peak = default_peak(rec, dtype) if peak is None else float(peak)
    if mse == 0:
        psnr = math.inf
    elif peak == 0:
        psnr = -math.inf
    else:
        psnr = 10.0 * math.log10(peak * peak / mse)
    if peak == 0:
        nrmse = math.inf if rmse > 0 else 0.0
    else:
        nrmse = rmse / peak
    return {'count': count, 'mismatch': rec['mismatch'], 'max_abs_error': rec['max_abs'], 'mse': mse, 'rmse': rmse,
            'psnr': psnr, 'nrmse': nrmse, 'value_range': value_range, 'peak': peak}


def compare(x, r, peak=None):
    return derive(record(x, r), np.asarray(x).dtype, peak)


class Unreachable(ValueError):
    pass


def search_quality(quality, L, target):
    """``(rung, probes)``: the coarsest-leaning rung of ``0 .. L - 1`` (0 the finest) that meets ``target``.

    1. ``quality(L - 1) >= target``: rung ``L - 1``.
    2. else ``quality(0) < target``: :class:`Unreachable`.
    3. else bisect with ``lo = 0`` (meets) and ``hi = L - 1`` (fails): ``mid = (lo + hi) // 2`` goes to ``lo``
       when it meets the target, else to ``hi``; stop at ``hi - lo == 1`` and take ``lo``.

    No monotonicity is assumed: the rung taken meets the target, its coarser neighbour does not (or does
    not exist), and at most ``2 + ceil(log2 L)`` rungs are probed."""
    probes = []

    def ask(k):
        probes.append((k, quality(k)))
        return probes[-1][1]
    if ask(L - 1) >= target:
        return L - 1, probes
    if L == 1 or not ask(0) >= target:
        raise Unreachable(probes[-1][1])
    lo, hi = 0, L - 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if ask(mid) >= target:
            lo = mid
        else:
            hi = mid
    return lo, probes
