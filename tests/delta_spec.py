"""Time series (delta coding along the batch axis), as a specification: pure numpy, knows nothing of the
product.  Shared by test_delta_spec.py (the rule, from numpy and the oracle alone) and the test_gpu_delta*.py
files (the kernels, ``kom.delta`` and the files).

The rule.  ``n`` is an integer array of shape ``(T, ...)`` and width W in {8, 16, 32}.  ``K`` is the key
interval: ``None`` means only frame 0 is a key frame, else ``K >= 1``; frame ``t`` is a key frame iff ``t == 0``
or (``K`` is not None and ``t % K == 0``).

    d[t] = n[t]                          key frame
    d[t] = (n[t] - n[t-1]) mod 2^W       otherwise

    n[t] = d[t]                          key frame
    n[t] = (d[t] + n[t-1]) mod 2^W       otherwise

``d`` is stored as the SIGNED type of width W (int8 for uint8 / int8, int16 for uint16 / int16, int32 for
int32); key frames of unsigned input are reinterpreted bit for bit.  A small negative delta is then a small
signed value.  Subsampling commutes with an elementwise delta, so level ``k`` of ``d`` is the delta of level
``k`` of ``n``.
"""

import numpy as np

DTYPES = (np.uint8, np.int8, np.uint16, np.int16, np.int32)
SIGNED = {np.dtype(np.uint8): np.dtype(np.int8), np.dtype(np.int8): np.dtype(np.int8),
          np.dtype(np.uint16): np.dtype(np.int16), np.dtype(np.int16): np.dtype(np.int16),
          np.dtype(np.int32): np.dtype(np.int32)}
UNSIGNED = {1: np.dtype(np.uint8), 2: np.dtype(np.uint16), 4: np.dtype(np.uint32)}


def check_key_interval(K):
    if K is None:
        return None
    if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or K < 1:
        raise ValueError(f'key_interval must be None or an int >= 1, got {K!r}')
    return int(K)


def is_key(t, K):
    return t == 0 or (K is not None and t % K == 0)


def _u(a):
    """``a`` as the unsigned type of its width: numpy's arithmetic on it is modulo 2^W."""
    a = np.ascontiguousarray(a)
    return a.view(UNSIGNED[a.dtype.itemsize])


def sub(x, pred):
    """What KMP_CODER_DELTA ENCODE writes: ``(x - pred) mod 2^W``, in ``x``'s dtype."""
    x = np.ascontiguousarray(x)
    return (_u(x) - _u(pred)).view(x.dtype)


def add(x, pred):
    """What KMP_CODER_DELTA DECODE writes: ``(x + pred) mod 2^W``, in ``x``'s dtype."""
    x = np.ascontiguousarray(x)
    return (_u(x) + _u(pred)).view(x.dtype)


def encode(n, K=None):
    """``d`` of ``n``, in the signed type of its width."""
    K = check_key_interval(K)
    n = np.ascontiguousarray(n)
    s = n.view(SIGNED[n.dtype])
    d = s.copy()
    for t in range(1, n.shape[0]):
        if not is_key(t, K):
            d[t] = sub(s[t], s[t - 1])
    return d


def decode(d, dtype, K=None):
    """``n`` of ``d`` (the signed type of ``dtype``'s width), as ``dtype``."""
    K = check_key_interval(K)
    d = np.ascontiguousarray(d)
    assert d.dtype == SIGNED[np.dtype(dtype)], (d.dtype, dtype)
    n = d.copy()
    for t in range(1, d.shape[0]):
        if not is_key(t, K):
            n[t] = add(d[t], n[t - 1])
    return n.view(np.dtype(dtype))


def level(a, ndim, k):
    """Pyramid level ``k`` of ``a = (T, spatial..., C...)``: every spatial axis strided by ``2**k``."""
    return a[(slice(None), *[slice(None, None, 2 ** k)] * ndim)]


def frames_read(a, b, K):
    """The frames a partial read of ``[a, b)`` decodes: from the key frame at or before ``a``."""
    return (a - a % K if K else 0), b


# ---------------------------------------------------------------------------------------------------
# the sequence the size figures are quoted on
# ---------------------------------------------------------------------------------------------------

SEED = 22
FRAMES, SHAPE = 6, (24, 28, 32)
# (cells the field advects by per frame, sigma of the fresh per-frame noise)
ROWS = ((0.0, 0.0), (0.05, 0.0), (0.25, 0.0), (1.0, 0.0), (0.05, 1 / 60), (0.25, 1 / 15))
EXPONENTS = (-10, -6, -3)
# the four sines: (amplitude, wavelength along z, y, x in cells; 0: constant along that axis)
SINES = ((1.0, 0, 0, 16), (0.7, 0, 14, 24), (0.5, 12, 0, 11), (0.3, 9, 13, 19))
TEXTURE_SIGMA = 1 / 15


def sequence(shift, noise, seed=SEED, frames=FRAMES, shape=SHAPE):
    """``(frames, *shape, 1)`` float32: four sines that advect along x by ``shift`` cells per frame, a frozen
    white texture of sigma 1/15 (the same in every frame) and fresh white noise of sigma ``noise`` per frame."""
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(*[np.arange(s, dtype=np.float64) for s in shape], indexing='ij')
    texture = rng.standard_normal(shape) * TEXTURE_SIGMA
    out = np.empty((frames, *shape, 1), np.float32)
    for t in range(frames):
        f = texture.copy()
        for amp, lz, ly, lx in SINES:
            phase = (z / lz if lz else 0.0) + (y / ly if ly else 0.0) + (x - shift * t) / lx
            f += amp * np.sin(2 * np.pi * phase)
        if noise:
            f += rng.standard_normal(shape) * noise
        out[t, ..., 0] = f
    return out


def size_row(shift, noise, e):
    """``(independent, delta)`` Rice bits per sample of the sequence quantised on the step ``2**e``: a 2-level
    MeanPredictor(0) pyramid (signed_spec.encode, oracle.rice.plan) of the integers and of their deltas."""
    import quant_spec
    n, exc = quant_spec.quantise(sequence(shift, noise), e)
    assert exc is None and n.dtype == np.int16
    return quant_spec.pyramid_bits(n, 3, 0, 2), quant_spec.pyramid_bits(encode(n), 3, 0, 2)
