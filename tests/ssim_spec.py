"""The structural similarity of a restored array against its original, in numpy: the rule the SSIM kernels,
``kom.metrics.ssim`` and ``compress(target_ssim=...)`` are tested against.

Inputs: ``x`` the original and ``r`` the restored array, one dtype among float32, uint8, uint16, int8, int16,
viewed as ``N`` independent items of ``D x H x W`` samples (``D = 1`` for images).  The window side is ``K = 7``,
``NP = 7^nsp`` with ``nsp = 2`` when ``D == 1`` and 3 otherwise; every spatial extent in use must be >= 7.

* Windows: only those that lie wholly inside one item -- ``(D - 6)(H - 6)(W - 6)`` per item (``(H - 6)(W - 6)``
  for images).  No padding: the set scikit-image keeps after its crop.
* Samples: integers enter as unsigned, int8 / int16 through ``M(v) = v ^ signbit``; ``base = 0``.  float32
  samples enter as ``double(v) - base`` with ``base`` the smallest finite original, a zero as ``+0.0``.  A float32
  window is SKIPPED iff one of its ``NP`` positions holds a non-finite ``x`` or ``r``.
* Per window, with ``Sx, Sr, Sxx, Srr, Sxr`` the sums of ``x, r, x^2, r^2, x r`` over its samples, in float64::

      mx = Sx / NP,  mr = Sr / NP
      vx  = (NP Sxx - Sx Sx) / (NP (NP - 1))          sample variance, scikit-image's default
      vr  = (NP Srr - Sr Sr) / (NP (NP - 1))
      vxr = (NP Sxr - Sx Sr) / (NP (NP - 1))
      C1 = (0.01 L)^2,  C2 = (0.03 L)^2
      s = ((2 mx mr + C1)(2 vxr + C2)) / ((mx^2 + mr^2 + C1)(vx + vr + C2))

  ``L`` is the peak: by default the range of the finite originals (float32) or ``2^W - 1``; ``L == 0`` has no SSIM
  (ValueError).
* The record: ``windows`` counted, ``skipped``, the sum of ``s`` over the counted windows and their minimum
  (``+inf`` when there are none).  ``ssim = sum / windows``, ``nan`` when ``windows == 0``.

The sums here are separable box sums of shifted slices (W, then H, then D), every window from its own terms.
For integer samples they are exact in float64 (``NP Sxx - Sx^2 < 2^50``).  For float32 samples in ``[0, L]`` a sum
of <= 343 terms carries <= 343 2^-53 relative error and the cancellation in ``NP Sxx - Sx^2`` is divided by at
least ``C2 = 9e-4 L^2``: about 4e-11 per window, so a device's mean is held to 1e-9 of this one, an integer one to
2^-40 (each ``s`` comes from about twenty roundings of quantities whose ratio is bounded by 1).
"""

import math

import numpy as np

K = 7
DTYPES = (np.float32, np.uint8, np.uint16, np.int8, np.int16)
TOL_INT, TOL_F32 = 2.0 ** -40, 1e-9


def mapped(a):
    """Integer samples as the unsigned integers they enter as (``M(v) = v ^ signbit`` for signed ones)."""
    a = np.asarray(a)
    if a.dtype.kind == 'i':
        u = a.view({1: np.uint8, 2: np.uint16}[a.dtype.itemsize])
        return u ^ u.dtype.type(1 << (8 * a.dtype.itemsize - 1))
    return a


def default_frame(x):
    """``(peak, base)`` of the original ``x``: its finite range and smallest finite value (float32), or
    ``2^W - 1`` and 0."""
    x = np.asarray(x)
    if x.dtype == np.float32:
        fin = x[np.isfinite(x)].astype(np.float64)
        if fin.size == 0:
            return 0.0, 0.0
        return float(fin.max() - fin.min()), float(fin.min()) + 0.0  # -0.0 + 0.0 is +0.0
    return float(2 ** (8 * x.dtype.itemsize) - 1), 0.0


def box(a, axes):
    """The sum of ``a`` over every window of side K along ``axes``: shifted slices, one axis after the other."""
    for ax in axes:
        n = a.shape[ax] - (K - 1)
        a = sum(np.take(a, range(k, k + n), axis=ax) for k in range(K))
    return a


def window_map(x, r, peak=None):
    """``(s, skipped mask, peak, base)``: the index of every window of the ``(N, D, H, W)`` arrays, shape
    ``(N, D', H - 6, W - 6)`` with ``D' = 1`` for images."""
    x, r = np.asarray(x), np.asarray(r)
    assert x.dtype == r.dtype and x.shape == r.shape and x.ndim == 4 and x.dtype in [np.dtype(d) for d in DTYPES]
    N, D, H, W = x.shape
    assert (D == 1 or D >= K) and H >= K and W >= K
    L, base = default_frame(x)
    L = L if peak is None else float(peak)
    if not L > 0 or not math.isfinite(L):
        raise ValueError(f'no SSIM for a peak of {L}')
    axes = (3, 2) if D == 1 else (3, 2, 1)
    NP = float(K ** len(axes))
    if x.dtype == np.float32:
        bad = ~(np.isfinite(x) & np.isfinite(r))
        xd = np.where(bad, 0.0, x.astype(np.float64) - base)
        rd = np.where(bad, 0.0, r.astype(np.float64) - base)
        skipped = box(bad.astype(np.int64), axes) > 0
    else:
        xd, rd = mapped(x).astype(np.float64), mapped(r).astype(np.float64)
        skipped = np.zeros(box(np.zeros(x.shape, np.int8), axes).shape, bool)
    Sx, Sr, Sxx, Srr, Sxr = (box(a, axes) for a in (xd, rd, xd * xd, rd * rd, xd * rd))
    mx, mr = Sx / NP, Sr / NP
    vx = (NP * Sxx - Sx * Sx) / (NP * (NP - 1))
    vr = (NP * Srr - Sr * Sr) / (NP * (NP - 1))
    vxr = (NP * Sxr - Sx * Sr) / (NP * (NP - 1))
    C1, C2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    s = ((2 * mx * mr + C1) * (2 * vxr + C2)) / ((mx * mx + mr * mr + C1) * (vx + vr + C2))
    return s, skipped, L, base


def ssim(x, r, peak=None):
    """``{'ssim', 'min_ssim', 'windows', 'skipped', 'sum', 'peak', 'base'}`` of ``(N, D, H, W)`` arrays."""
    s, skipped, L, base = window_map(x, r, peak)
    kept = s[~skipped]
    windows = int(kept.size)
    total = math.fsum(kept.tolist())
    return {'ssim': total / windows if windows else math.nan, 'min_ssim': float(kept.min()) if windows else math.inf,
            'windows': windows, 'skipped': int(skipped.sum()), 'sum': total, 'peak': L, 'base': base}


def items(a):
    """An array in the package's layouts ``(B, H, W, C)`` / ``(B, D, H, W, C)`` as ``(N, D, H, W)`` items,
    channels first."""
    a = np.asarray(a)
    assert a.ndim in (4, 5)
    a = np.moveaxis(a, -1, 1)
    a = a.reshape((a.shape[0] * a.shape[1],) + a.shape[2:])
    return np.ascontiguousarray(a[:, None] if a.ndim == 3 else a)


def windows_per_item(D, H, W):
    return (1 if D == 1 else D - 6) * (H - 6) * (W - 6)
