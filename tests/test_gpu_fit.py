"""``linear_moments`` (kmp_fit.hip) bit for bit against its numpy specification, its extreme values
against closed forms, and ``LinearPredictor.fit`` end to end through the codecs and the container."""

import functools

import numpy as np
import pytest
import torch

import oracle
from oracle import predictors as OP
from fit_spec import PROBES, PROBE_IDS, PROBE_SEED, field, mean_abs_residual, ns_of, spec_moments

pytestmark = pytest.mark.gpu

VOLUMES = [(1, 3, 3, 3, 1), (2, 5, 4, 7, 1), (1, 9, 14, 130, 1), (3, 17, 30, 16, 1), (2, 64, 64, 64, 1)]
IMAGES = [(2, 3, 3, 1), (1, 37, 70, 1), (2, 256, 256, 1)]
CASES = [(3, s, p) for s in VOLUMES for p in (0, 1)] + [(2, s, p) for s in IMAGES for p in (0, 1, 2)]


@functools.lru_cache(maxsize=None)
def _random(shape, dtype):
    """Full-range random samples (shared, never modified)."""
    rng = np.random.default_rng(sum(shape) * 131 + np.dtype(dtype).itemsize)
    a = rng.integers(0, np.iinfo(dtype).max + 1, size=shape, dtype=np.int64).astype(dtype)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _spec(shape, dtype, p, ndim):
    m = spec_moments(_random(shape, dtype), p, ndim)
    m.setflags(write=False)
    return m


@pytest.mark.parametrize('dtype', [np.uint8, np.uint16], ids=['u8', 'u16'])
@pytest.mark.parametrize('ndim,shape,p', CASES, ids=[f'{n}d-{"x".join(map(str, s))}-p{p}' for n, s, p in CASES])
def test_moments_bit_equal_to_the_specification(kom, ndim, shape, p, dtype):
    h = _random(shape, dtype)
    want = _spec(shape, dtype, p, ndim)
    got = kom.linear_moments(h, p, ndim)
    assert got.dtype == np.int64 and got.shape == want.shape
    bad = np.argwhere(got != want)
    assert bad.size == 0, f'{len(bad)} of {want.size} entries differ, first {bad[:4].tolist()}'
    got_t = kom.linear_moments(torch.from_numpy(h.copy()).cuda(), p, ndim)
    assert isinstance(got_t, np.ndarray) and np.array_equal(got_t, want)


def _closed_form(values, n):
    """M = n v v^T for columns that are constant over all n cells (v ends with the constant 1)."""
    v = np.array(list(values) + [1], dtype=object)
    return np.outer(v, v) * n


def _as_i64(m):
    assert all(-2 ** 63 <= int(x) < 2 ** 63 for x in m.ravel())
    return m.astype(np.int64)


@pytest.mark.parametrize('p', [0, 1])
@pytest.mark.parametrize('value', [0, 0xFFFF], ids=['all0', 'allmax'])
def test_constant_extremes_match_the_closed_form(kom, value, p):
    shape = (8, 64, 64, 64, 1)
    n = 8 * 32 ** 3
    h = torch.full(shape, value - 0x10000 if value > 0x7FFF else value, dtype=torch.int16, device='cuda').view(torch.uint16)
    got = kom.linear_moments(h, p, 3)
    assert np.array_equal(got, _as_i64(_closed_form([value] * ((2 * p + 2) ** 3 + 19), n)))


@pytest.mark.parametrize('p', [0, 1])
def test_checkerboard_matches_the_closed_form(kom, p):
    """0 / 0xFFFF by the parity of z + y + x: every lowres node (even coordinates, mirrored ones
    included) is 0, every target with an odd number of odd coordinates is 0xFFFF -- C, z0..3, y0..3,
    x0..3 -- and L, R, U, D, F, B are 0.  Mixed-sign biased bytes (-128 and 127) in one product."""
    z, y, x = np.ogrid[:64, :64, :64]
    one = (((z + y + x) & 1) * 0xFFFF).astype(np.uint16)
    h = np.broadcast_to(one[None, ..., None], (8, 64, 64, 64, 1)).copy()
    cols = [0] * (2 * p + 2) ** 3 + [0] * 6 + [0xFFFF] * 13
    got = kom.linear_moments(h, p, 3)
    assert np.array_equal(got, _as_i64(_closed_form(cols, 8 * 32 ** 3)))


def test_sum_of_squares_beyond_2_53_is_exact(kom):
    """All-0xFFFF over 72 x 32^3 = 2.36 M cells: sum f^2 = 1.013e16 > 2^53, so any float64 on the
    path (kernel, finisher, or the Python wrapper) loses its low bits."""
    n = 72 * 32 ** 3
    assert n * 0xFFFF ** 2 > 2 ** 53
    h = torch.full((72, 64, 64, 64, 1), -1, dtype=torch.int16, device='cuda').view(torch.uint16)
    got = kom.linear_moments(h, 1, 3)
    assert np.array_equal(got, _as_i64(_closed_form([0xFFFF] * 83, n)))


def test_accumulators_are_flushed_before_they_overflow(kom):
    """The work split (kmp_fit.hip): at most kFitGrid = 512 workgroups, each taking one contiguous run
    of 64-cell steps; a wave keeps one i32 accumulator tile per block pair for the whole run and
    adds it to the int64 table every kFlushSteps = 1024 steps.  With all-0xFFFF samples every biased
    byte is 127, so a byte x byte accumulator element grows by 64 * 127^2 = 1,032,256 per step and
    would pass 2^31 after 2080.4 steps.  At (8,64,64,64,1) and (72,64,64,64,1) a workgroup's run is
    only 8 and 72 steps, so those sizes cannot show a missing flush; this batch is enlarged until
    one can: 2100 volumes = 1,075,200 steps = 2100 steps per workgroup, 2100 * 1,032,256 =
    2.168e9 > 2^31 = 2.147e9 in every byte x byte accumulator of every workgroup."""
    B = 2100
    steps_per_group = B * 32 ** 3 // 64 // 512
    assert steps_per_group * 64 * 127 * 127 > 2 ** 31
    h = torch.full((B, 64, 64, 64, 1), -1, dtype=torch.int16, device='cuda').view(torch.uint16)
    got = kom.linear_moments(h, 0, 3)
    assert np.array_equal(got, _as_i64(_closed_form([0xFFFF] * 27, B * 32 ** 3)))


@pytest.mark.parametrize('ndim,shape,p', [(3, (3, 17, 30, 16, 1), 1), (2, (2, 256, 256, 1), 2)], ids=['3d', '2d'])
def test_deterministic_and_additive_over_the_batch(kom, ndim, shape, p):
    B = shape[0] + 1
    h = _random((B,) + shape[1:], np.uint16)
    a, b = kom.linear_moments(h, p, ndim), kom.linear_moments(h, p, ndim)
    assert np.array_equal(a, b)
    assert np.array_equal(a, kom.linear_moments(h[:1], p, ndim) + kom.linear_moments(h[1:], p, ndim))


@functools.lru_cache(maxsize=None)
def _probe(i):
    ndim, shape, dtype, p = PROBES[i]
    h = field(shape, PROBE_SEED, dtype)
    h.setflags(write=False)
    return h


@pytest.mark.parametrize('i', range(len(PROBES)), ids=PROBE_IDS)
def test_fit_weights_are_solve_moments_of_the_specification(kom, i):
    ndim, shape, dtype, p = PROBES[i]
    h = _probe(i)
    w, b = kom.solve_moments(spec_moments(h, p, ndim), (2 * p + 2) ** ndim)
    pred = kom.LinearPredictor.fit(h, p, ndim)
    assert np.array_equal(pred.weights.numpy(), w) and np.array_equal(pred.bias.numpy(), b)
    # an iterable of arrays fits as the sum of their moments
    halves = kom.LinearPredictor.fit([h[:1], torch.from_numpy(h[1:].copy()).cuda()], p, ndim)
    assert np.array_equal(halves.weights.numpy(), w) and np.array_equal(halves.bias.numpy(), b)


@pytest.mark.parametrize('i', range(len(PROBES)), ids=PROBE_IDS)
def test_fitted_f32_predictor_codes_losslessly_like_the_oracle_and_beats_the_mean(kom, i):
    ndim, shape, dtype, p = PROBES[i]
    h = _probe(i)
    bits = 8 * np.dtype(dtype).itemsize
    api, ons = (kom.volume, oracle.volume) if ndim == 3 else (kom.image, oracle.image)
    enc, dec = getattr(api, f'encode_values_uint{bits}'), getattr(api, f'decode_values_uint{bits}')
    oenc = getattr(ons, f'encode_values_uint{bits}')
    pred = kom.LinearPredictor.fit(h, p, ndim, arith='f32')
    lo, (maps, dims) = api.encode(pred, enc, h, padding=p)
    assert np.array_equal(api.decode(pred, dec, lo, (maps, dims), padding=p), h)
    fn = OP.linear_predictions_fn(p, pred.weights.numpy(), pred.bias.numpy(), ndim)
    olo, (omaps, odims) = ons.encode(fn, oenc, h, p)
    assert tuple(dims) == tuple(odims) and np.array_equal(lo, olo)
    assert all(np.array_equal(a, b) for a, b in zip(maps, omaps))
    mean = kom.MeanPredictor(p, ndim)
    _, (mmaps, _) = api.encode(mean, enc, h, padding=p)
    fitted, base = mean_abs_residual(maps, bits), mean_abs_residual(mmaps, bits)
    print(f'mean |residual|: MeanPredictor {base:.3f}, fitted {fitted:.3f}')
    assert fitted < base


def test_auto_arithmetic_round_trips_through_the_container_and_is_smaller(kom, tmp_path):
    # 3D uint16 padding 1: 'auto' is the matrix-core bf16x2 form.  A probe field of 8 times the
    # samples: the file records the 64 x 19 weights as text (~25 KB), more than a better prediction
    # can save on the 55 KB of the (2, 24, 22, 26) probe.
    ndim, p = 3, 1
    h = field((2, 48, 44, 52), PROBE_SEED, np.uint16)
    pred = kom.LinearPredictor.fit(h, p, ndim)
    assert pred.arith == 'auto' and pred.arith_for(torch.uint16) == 'bf16x2'
    fitted = kom.container.compress(str(tmp_path / 'fit.kmp'), h, pred)
    assert np.array_equal(kom.container.decompress(str(tmp_path / 'fit.kmp')), h)
    base = kom.container.compress(str(tmp_path / 'mean.kmp'), h, kom.MeanPredictor(p, ndim))
    print(f"file bytes: MeanPredictor {base['bytes']}, fitted {fitted['bytes']}")
    assert fitted['bytes'] < base['bytes']
