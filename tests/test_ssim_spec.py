"""tests/ssim_spec.py against scikit-image's formula written with scipy's uniform filter, its closed forms, its
window rules and the figures DESIGN.md §23 quotes for the spec field (CPU only)."""

import math

import numpy as np
import pytest

import quant_spec as Q
import ssim_spec as S


def uniform_filter_ssim(x, r, L):
    """scikit-image's structural_similarity (win_size 7, uniform weights, sample covariance, the crop of
    3 samples per side) on one item of float64 samples: the mean and the map."""
    from scipy.ndimage import uniform_filter
    NP = 7 ** x.ndim
    cov_norm = NP / (NP - 1)
    ux, ur = uniform_filter(x, 7), uniform_filter(r, 7)
    uxx, urr, uxr = uniform_filter(x * x, 7), uniform_filter(r * r, 7), uniform_filter(x * r, 7)
    vx, vr, vxr = cov_norm * (uxx - ux * ux), cov_norm * (urr - ur * ur), cov_norm * (uxr - ux * ur)
    C1, C2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    s = ((2 * ux * ur + C1) * (2 * vxr + C2)) / ((ux ** 2 + ur ** 2 + C1) * (vx + vr + C2))
    crop = s[tuple(slice(3, -3) for _ in range(x.ndim))]
    return crop.mean(), crop


@pytest.mark.parametrize('dtype,shape', [(np.uint8, (1, 15, 22)), (np.uint16, (12, 20, 24))],
                         ids=['uint8-2d', 'uint16-3d'])
def test_agrees_with_the_uniform_filter_form(dtype, shape):
    pytest.importorskip('scipy')
    rng = np.random.default_rng(3)
    top = np.iinfo(dtype).max
    x = rng.integers(0, top + 1, size=shape).astype(dtype)
    r = np.clip(x.astype(np.int64) + rng.integers(-top // 8, top // 8 + 1, size=shape), 0, top).astype(dtype)
    got = S.ssim(x[None], r[None])
    s_map = S.window_map(x[None], r[None])[0][0]
    xf, rf = x.astype(np.float64), r.astype(np.float64)
    if shape[0] == 1:
        xf, rf, s_map = xf[0], rf[0], s_map[0]
    mean, crop = uniform_filter_ssim(xf, rf, float(top))
    assert crop.shape == s_map.shape and got['windows'] == crop.size == S.windows_per_item(*shape)
    print(f'{np.dtype(dtype).name}: spec {got["ssim"]!r}, uniform filter {mean!r}, max map gap {np.abs(crop - s_map).max():.3g}')
    assert abs(got['ssim'] - mean) <= 1e-12 and np.abs(crop - s_map).max() <= 1e-12


@pytest.mark.parametrize('dtype', S.DTYPES, ids=[np.dtype(d).name for d in S.DTYPES])
def test_identical_arrays_give_exactly_one(dtype):
    rng = np.random.default_rng(1)
    for shape in ((2, 1, 9, 11), (2, 8, 9, 10)):
        if dtype == np.float32:
            x = rng.standard_normal(shape).astype(np.float32)
        else:
            info = np.iinfo(dtype)
            x = rng.integers(info.min, int(info.max) + 1, size=shape).astype(dtype)
        got = S.ssim(x, x.copy())
        assert got['ssim'] == 1.0 and got['min_ssim'] == 1.0 and got['skipped'] == 0
        assert got['windows'] == shape[0] * S.windows_per_item(*shape[1:])


def test_two_constant_arrays_match_the_closed_form():
    """No variance on either side: s = (2 a b + C1) / (a^2 + b^2 + C1) in every window."""
    for dtype, a, b in ((np.uint8, 200, 180), (np.uint16, 1000, 50000), (np.int8, -100, 27), (np.int16, -5, 5)):
        x, r = np.full((1, 7, 8, 9), a, dtype), np.full((1, 7, 8, 9), b, dtype)
        L = float(2 ** (8 * np.dtype(dtype).itemsize) - 1)
        am, bm = float(S.mapped(x)[0, 0, 0, 0]), float(S.mapped(r)[0, 0, 0, 0])
        C1 = (0.01 * L) ** 2
        want = (2 * am * bm + C1) / (am * am + bm * bm + C1)
        got = S.ssim(x, r)
        assert got['windows'] == 6 and abs(got['ssim'] - want) <= 2.0 ** -50 and abs(got['min_ssim'] - want) <= 2.0 ** -50
    # float32: the base is the original's value, so x enters as 0 and r as b - a; the peak must be given
    x, r = np.full((1, 1, 7, 7), 3.0, np.float32), np.full((1, 1, 7, 7), 3.5, np.float32)
    C1 = (0.01 * 2.0) ** 2
    assert abs(S.ssim(x, r, peak=2.0)['ssim'] - C1 / (0.25 + C1)) <= 2.0 ** -50
    with pytest.raises(ValueError):
        S.ssim(x, r)  # L == 0: no SSIM


def test_a_nan_skips_exactly_the_windows_that_contain_it():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((2, 10, 12, 13)).astype(np.float32)
    r = (x + rng.standard_normal(x.shape).astype(np.float32) * np.float32(0.01)).astype(np.float32)
    clean = S.window_map(x, r)
    for side in ('x', 'r'):
        for at in ((1, 4, 5, 6), (0, 0, 0, 0), (1, 9, 11, 12)):
            xx, rr = x.copy(), r.copy()
            (xx if side == 'x' else rr)[at] = np.nan
            s, skipped, _, _ = S.window_map(xx, rr)
            want = np.zeros(skipped.shape, bool)
            n, z, y, w = at
            want[n, max(0, z - 6):z + 1, max(0, y - 6):y + 1, max(0, w - 6):w + 1] = True
            assert np.array_equal(skipped, want)
            got = S.ssim(xx, rr)
            assert got['skipped'] == want.sum() and got['windows'] == want.size - want.sum()
            if (xx if side == 'x' else rr) is rr:  # the frame of the original is unchanged: the others are bit-equal
                assert np.array_equal(s[~want], clean[0][~want])
    assert math.isnan(S.ssim(np.full((1, 1, 7, 7), np.nan, np.float32), np.zeros((1, 1, 7, 7), np.float32), peak=1)['ssim'])


def test_signed_samples_equal_the_mapped_unsigned_ones():
    rng = np.random.default_rng(9)
    for sd, ud in ((np.int8, np.uint8), (np.int16, np.uint16)):
        info = np.iinfo(sd)
        x = rng.integers(info.min, int(info.max) + 1, size=(2, 7, 9, 8)).astype(sd)
        r = np.clip(x.astype(np.int64) + rng.integers(-9, 10, size=x.shape), info.min, info.max).astype(sd)
        xu, ru = S.mapped(x), S.mapped(r)
        assert xu.dtype == ud and int(xu.min()) >= 0 and np.array_equal(np.argsort(x, None, 'stable'), np.argsort(xu, None, 'stable'))
        assert S.ssim(x, r) == S.ssim(xu, ru)


def test_the_spec_field_table():
    """The figures DESIGN.md §23 quotes: SSIM strictly decreasing over e = -12 .. 2, and 0.99 between e = -4 and
    e = -3, so ``target_ssim = 0.99`` picks e = -4."""
    import metrics_spec as M
    x = Q.spec_field()
    xi = S.items(x)
    rows = {}
    for e in range(-12, 3):
        n, exc = Q.quantise(x, e)
        r = Q.restore(n, e, exc)
        rows[e] = (S.ssim(xi, S.items(r))['ssim'], M.compare(x, r)['psnr'])
        print(f'e = {e:3d}   ssim = {rows[e][0]:.9f}   psnr = {rows[e][1]:.1f} dB')
    values = [rows[e][0] for e in range(-12, 3)]
    assert all(a > b for a, b in zip(values, values[1:]))
    assert rows[-4][0] >= 0.99 > rows[-3][0]
    quoted = {-8: 0.9999866, -6: 0.9997859, -5: 0.9991459, -4: 0.9965820, -3: 0.9865416, -2: 0.949088, -1: 0.835875,
              0: 0.506475}
    for e, v in quoted.items():
        assert abs(rows[e][0] - v) <= 5e-7, (e, rows[e][0], v)
