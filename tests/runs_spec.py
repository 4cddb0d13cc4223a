"""Masked float32 fields in numpy: exception runs and the hold-fill, the rule ``kom.quant``, the
``KMP_CODER_FILL`` / ``KMP_CODER_RUNS`` kernels and the version-7 container are tested against.

**Runs.**  The exceptions of ``quant_spec`` / ``prec_spec`` are flat int64 indices ascending and uint32 bits.
A run is a maximal stretch of consecutive indices whose bits are all equal, cut so that no run is longer
than ``cap = 2**32 - 1``.  Run ``j`` has ``start_j``, ``length_j >= 1`` and ``bits_j``; the stored form is four
uint32 arrays of ``R`` entries: the low and the high words of ``start_j - start_{j-1}`` (``start_{-1} = 0``, the
encoding of ``quant_spec.gaps_from_indices`` on the starts), ``length_j``, and ``bits_j - bits_{j-1}`` modulo
``2**32`` (``bits_{-1} = 0``).

**Fill.**  In an integer array whose exceptions are marked by the type's minimum (what the quantising
``kmp_code`` ENCODE writes), every marked element takes the value of the last unmarked element before it in
flat C order; the marked elements before the first unmarked one take that first value; an array with no
unmarked element becomes all 0; unmarked elements are unchanged.
"""

import numpy as np

import quant_spec

CAP = 2 ** 32 - 1


def runs_from_exceptions(idx, bits, cap=CAP):
    """``(starts int64, lengths int64, bits uint32)`` of the maximal runs, none longer than ``cap``."""
    idx, bits = np.asarray(idx, np.int64), np.asarray(bits, np.uint32)
    assert idx.shape == bits.shape and idx.ndim == 1 and cap >= 1
    if idx.size == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.uint32)
    new = np.ones(idx.size, bool)
    new[1:] = (np.diff(idx) != 1) | (bits[1:] != bits[:-1])
    first = np.flatnonzero(new)
    starts, lengths, rbits = [], [], []
    for s, e in zip(first, [*first[1:], idx.size]):
        for at in range(int(s), int(e), cap):
            starts.append(int(idx[at]))
            lengths.append(min(cap, int(e) - at))
            rbits.append(int(bits[s]))
    return np.array(starts, np.int64), np.array(lengths, np.int64), np.array(rbits, np.uint32)


def runs(exceptions, cap=CAP):
    """The four stored uint32 arrays ``(start gaps low, high, lengths, bit deltas)`` of ``(indices, bits)``."""
    starts, lengths, rbits = runs_from_exceptions(*exceptions, cap=cap)
    lo, hi = quant_spec.gaps_from_indices(starts)
    delta = np.diff(rbits.astype(np.int64), prepend=np.int64(0)) % (1 << 32)
    return lo, hi, lengths.astype(np.uint32), delta.astype(np.uint32)


def starts_bits(lo, hi, lengths, delta):
    """``(starts int64, lengths int64, bits uint32)`` of the stored arrays."""
    starts = quant_spec.indices_from_gaps(np.asarray(lo, np.uint32), np.asarray(hi, np.uint32))
    bits = (np.cumsum(np.asarray(delta, np.uint32).astype(np.int64)) % (1 << 32)).astype(np.uint32)
    return starts, np.asarray(lengths, np.uint32).astype(np.int64), bits


def exceptions_from_runs(lo, hi, lengths, delta):
    """``(indices int64 ascending, bits uint32)``: the runs expanded."""
    starts, lengths, bits = starts_bits(lo, hi, lengths, delta)
    total = int(lengths.sum())
    within = np.arange(total, dtype=np.int64) - np.repeat(np.cumsum(lengths) - lengths, lengths)
    return np.repeat(starts, lengths) + within, np.repeat(bits, lengths)


def mark(dtype):
    return np.iinfo(dtype).min


def fill(n):
    """The hold-fill of the marked integer array ``n`` (a new array of the same shape and dtype)."""
    n = np.asarray(n)
    flat = n.reshape(-1)
    ok = flat != mark(n.dtype)
    if not ok.any():
        return np.zeros_like(n)
    at = np.where(ok, np.arange(flat.size), -1)
    src = np.maximum.accumulate(at)
    src[src < 0] = np.flatnonzero(ok)[0]
    return flat[src].reshape(n.shape)


def marked(n, exceptions):
    """``n`` (0 at the exceptions, as ``quantise`` returns it) with the exceptions marked."""
    out = np.array(n, copy=True)
    if exceptions is not None:
        out.reshape(-1)[exceptions[0]] = mark(out.dtype)
    return out


def extent(n, ok):
    """``(min, max)`` over the elements of ``n`` where ``ok`` (``(0, 0)`` where there are none)."""
    v = np.asarray(n)[ok]
    return (int(v.min()), int(v.max())) if v.size else (0, 0)
