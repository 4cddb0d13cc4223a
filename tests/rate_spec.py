"""Rate control, the specification, in plain Python: the budget, the ladders, the
search and the sized quantity.  Independent of the product: the tests compare ``kompressor_amd.rate``
and ``container.compress(target_bits=...)`` with it.

Ladders run from the finest rung to the coarsest:

* 'abs': step exponents ``e`` (``abs_error = 2**(e - 1)``); with ``M`` the largest finite ``|x|`` and
  ``ex = frexp(M)[1]``, ``e = clamp(ex - 30) .. clamp(ex + 1)`` clamped to [-126, 127]; ``M = 0`` or no
  finite value: the single rung 0.
* 'rel': kept mantissa bits ``m = 22 .. 0`` (``rel_error = 2**-(m + 1)``).
* 'near': ``max_error = 0 .. 2**(W - 1) - 1``.

``search(size, L, budget) -> (rung, probes)``:

1. ``size(0) <= budget``: rung 0.
2. else ``size(L - 1) > budget``: ValueError.
3. else bisect from ``lo = 0`` (too big), ``hi = L - 1`` (fits): ``mid = (lo + hi) // 2``; ``hi = mid`` if
   ``size(mid) <= budget`` else ``lo = mid``; stop at ``hi - lo == 1`` and take ``hi``.

Without assuming monotone sizes: the chosen rung fits, the next finer rung does not, and at most
``2 + ceil(log2 L)`` rungs are probed.
"""

import json
import math
import struct

import numpy as np

E_MIN, E_MAX = -126, 127
HEAD = struct.Struct('<4sHHQ')
WIDEST_CRC = 4294967295


def budget(numel, raw_bytes, target_bits=None, target_ratio=None):
    if target_bits is not None:
        return int(math.floor(target_bits * numel / 8))
    return int(math.floor(raw_bytes / target_ratio))


def ladder_abs(M):
    M = float(M)
    if not math.isfinite(M) or M <= 0:
        return [0]
    ex = math.frexp(M)[1]
    lo, hi = (min(max(e, E_MIN), E_MAX) for e in (ex - 30, ex + 1))
    return list(range(lo, hi + 1))


def largest_finite(x):
    a = np.abs(np.asarray(x, np.float64))
    a = a[np.isfinite(a)]
    return float(a.max()) if a.size else 0.0


def ladder_rel():
    return list(range(22, -1, -1))


def ladder_near(dtype):
    return list(range(0, 2 ** (8 * np.dtype(dtype).itemsize - 1)))


def bound_kw(mode, value):
    """The explicit-bound keyword of ``compress`` that codes a rung value."""
    if mode == 'abs':
        return {'abs_error': 2.0 ** (value - 1)}
    if mode == 'rel':
        return {'rel_error': 2.0 ** -(value + 1)}
    return {'max_error': int(value)}


def max_probes(L):
    return 2 + (math.ceil(math.log2(L)) if L > 1 else 0)


def search(size, L, budget):
    probes = []

    def ask(r):
        probes.append((r, size(r)))
        return probes[-1][1]
    if ask(0) <= budget:
        return 0, probes
    if L == 1 or ask(L - 1) > budget:
        raise ValueError(f'no rung fits {budget} bytes: the coarsest needs {probes[-1][1]}')
    lo, hi = 0, L - 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if ask(mid) <= budget:
            hi = mid
        else:
            lo = mid
    return hi, probes


def bound_bytes_of(path):
    """``bound_bytes`` of a written file: its length with the metadata serialised again (the same
    separators, the same padding to 8) under the widest ``crc32``, 4294967295."""
    with open(path, 'rb') as f:
        data = f.read()
    magic, version, _, meta_len = HEAD.unpack(data[:HEAD.size])
    assert magic == b'KMPF'
    stored = data[HEAD.size:HEAD.size + meta_len]
    meta = json.loads(stored)
    again = json.dumps(meta, separators=(',', ':')).encode()
    again += b' ' * (-len(again) % 8)
    assert again == stored, 'the metadata does not serialise back to its stored bytes'
    meta['crc32'] = WIDEST_CRC
    wide = json.dumps(meta, separators=(',', ':')).encode()
    wide += b' ' * (-len(wide) % 8)
    return len(data) - len(stored) + len(wide)
