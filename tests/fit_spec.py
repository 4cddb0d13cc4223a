"""The numpy specification of ``linear_moments`` and the seeded probe fields, shared by
test_fit_host.py and test_gpu_fit.py (the existing oracle functions, unchanged)."""

import numpy as np

import oracle


def ns_of(ndim):
    return oracle.volume if ndim == 3 else oracle.image


def design(h, p, ndim):
    """``X [B * cells, Q]`` int64: N features (z-major / y / x), K targets (reference order), 1 --
    the cells, and the feature windows, ``encode`` evaluates the predictor on."""
    ns = ns_of(ndim)
    hp, _ = ns.pad_highres(h)
    lo = ns.lowres_from_highres(hp)
    F = ns.features_from_lowres(ns.pad_neighborhood(lo, p), p)[..., 0]
    T = ns.targets_from_highres(hp)[..., 0]
    N, K = F.shape[-1], T.shape[-1]
    F, T = F.reshape(-1, N), T.reshape(-1, K)
    return np.concatenate([F, T, np.ones((F.shape[0], 1), F.dtype)], axis=1).astype(np.int64), N, K


def spec_moments(h, p, ndim):
    """``M = X^T X`` [Q, Q] int64, exact.  Taken through the float64 BLAS in runs of 2^20 rows: every
    partial sum of a run is an integer below 2^32 * 2^20 = 2^52, so float64 holds it exactly in
    any order (numpy's own int64 matmul is a slow scalar loop); the runs add in int64."""
    X, _, _ = design(h, p, ndim)
    M = np.zeros((X.shape[1],) * 2, np.int64)
    for r in range(0, X.shape[0], 1 << 20):
        Xf = X[r:r + (1 << 20)].astype(np.float64)
        M += (Xf.T @ Xf).astype(np.int64)
    return M


def field(shape, seed, dtype):
    """A smoothed random field plus noise, ``[*shape, 1]``."""
    r = np.random.default_rng(seed)
    x = r.standard_normal(shape)
    for ax in range(1, len(shape)):
        for _ in range(3):
            x = (x + np.roll(x, 1, ax) + np.roll(x, -1, ax) + np.roll(x, 2, ax)) / 4
    x = (x - x.min()) / (x.max() - x.min())
    top = 200 if dtype == np.uint8 else 40000
    sig = 1.5 if dtype == np.uint8 else 12.0
    return np.clip(x * top + 20 + r.standard_normal(shape) * sig, 0, np.iinfo(dtype).max).astype(dtype)[..., None]


# (ndim, shape without the channel axis, dtype, padding): the five probe cases, seed 7
PROBES = [(3, (2, 24, 22, 26), np.uint16, 0), (3, (2, 24, 22, 26), np.uint16, 1), (3, (2, 20, 20, 20), np.uint8, 1),
          (2, (2, 48, 50), np.uint8, 0), (2, (2, 48, 50), np.uint16, 1)]
PROBE_SEED = 7
PROBE_IDS = [f'{n}d-{np.dtype(d).name}-p{p}' for n, _, d, p in PROBES]


def mean_abs_residual(maps, bits):
    """Mean |signed residual| over all coded maps (modular residuals read as signed)."""
    tot = n = 0
    for m in maps:
        r = np.asarray(m).astype(np.int64)
        r = np.where(r >= 1 << (bits - 1), r - (1 << bits), r)
        tot += np.abs(r).sum()
        n += r.size
    return tot / n
