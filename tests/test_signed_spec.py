"""The signed-sample specification (tests/signed_spec.py) against the oracle alone: no GPU, no product."""

import numpy as np
import pytest

import oracle
import signed_spec as S
from conftest import golden_maps, load_golden


@pytest.mark.parametrize('dtype', S.SIGNED)
def test_map_round_trips_every_pattern_and_keeps_order(dtype):
    info = np.iinfo(dtype)
    x = np.arange(info.min, int(info.max) + 1, dtype=np.int64).astype(dtype)
    u = S.M(x)
    assert u.dtype == S.unsigned_of(dtype)
    assert np.array_equal(u.astype(np.int64), x.astype(np.int64) + S.signbit(dtype))  # x + 2^(W-1)
    assert np.all(np.diff(u.astype(np.int64)) == 1)                                   # order preserved
    assert np.array_equal(S.Minv(u), x)
    assert S.Minv(u).dtype == np.dtype(dtype)


@pytest.mark.parametrize('dtype', S.SIGNED)
def test_coder_is_the_signed_difference_mod_2w_and_inverts(dtype):
    gt, pred = S.uniform((4096,), dtype, 1), S.uniform((4096,), dtype, 2)
    gt[:5], pred[:5] = S.extremes(dtype), S.extremes(dtype)[::-1]
    enc = S.encode_values(pred, gt)
    enc_u, dec_u = S.unsigned_coders(dtype)
    # the map cancels: the unsigned coder on the mapped operands, and on the raw bit patterns
    assert np.array_equal(enc, enc_u(S.M(pred), S.M(gt)))
    assert np.array_equal(enc, enc_u(pred.view(enc.dtype), gt.view(enc.dtype)))
    assert np.array_equal(S.decode_values(pred, enc, dtype), gt)


@pytest.mark.parametrize('dtype', S.SIGNED)
@pytest.mark.parametrize('ndim,shape', [(3, (2, 7, 8, 9, 1)), (2, (2, 9, 12, 2))])
@pytest.mark.parametrize('padding', [0, 1])
def test_constant_minus_one_gives_zero_maps(dtype, ndim, shape, padding):
    x = np.full(shape, -1, dtype)
    lo, maps, dims = S.encode(x, S.mean_fn(padding, ndim), ndim, padding)
    assert lo.dtype == np.dtype(dtype) and np.all(lo == -1)
    for m in maps:
        assert m.dtype == S.unsigned_of(dtype) and not m.any()


@pytest.mark.parametrize('dtype', S.SIGNED)
@pytest.mark.parametrize('ndim,shape', [(3, (2, 9, 10, 12, 1)), (2, (2, 13, 16, 1))])
@pytest.mark.parametrize('padding', [0, 1])
def test_maps_equal_the_oracles_for_the_shifted_array(dtype, ndim, shape, padding):
    x = S.data(shape, dtype, seed=2)
    for v in S.extremes(dtype):
        assert (x == v).any()
    fn = S.mean_fn(padding, ndim)
    lo, maps, dims = S.encode(x, fn, ndim, padding)
    u = (x.astype(np.int64) + S.signbit(dtype)).astype(S.unsigned_of(dtype))  # x + 2^(W-1)
    enc, _ = S.unsigned_coders(dtype)
    lo_u, (maps_u, dims_u) = S.ons(ndim).encode(fn, enc, u, padding=padding)
    assert tuple(dims_u) == dims
    for a, b in zip(maps, maps_u):
        assert np.array_equal(a, b)
    sl = (slice(None),) + (slice(None, None, 2),) * ndim
    assert np.array_equal(lo, x[sl]) and lo.dtype == x.dtype
    assert np.array_equal(S.decode(lo, maps, dims, fn, ndim, padding), x)


def test_offset_coding_beats_the_bit_cast_on_a_zero_crossing_field():
    x = S.zero_crossing((1, 32, 32, 32, 1), np.int16, seed=0)
    neg = float((x < 0).mean())
    assert 0.5 < neg < 0.7, neg
    fn = S.mean_fn(0, 3)
    _, maps_off, _ = S.encode(x, fn, 3, 0)
    _, (maps_cast, _) = oracle.volume.encode(fn, oracle.common.encode_values_uint16, x.view(np.uint16), padding=0)
    off, cast = S.rice_bits_per_sample(maps_off), S.rice_bits_per_sample(maps_cast)
    print(f'Rice bits per residual sample: offset-binary {off:.2f}, bit-cast {cast:.2f}; {100 * neg:.0f} % negative')
    assert off < cast
    assert off < 8.0


def test_predictions_are_the_unmapped_unsigned_predictions():
    x = S.data((1, 6, 7, 8, 1), np.int16, seed=4)
    maps = S.predictions(x, S.mean_fn(0, 3))
    want = S.mean_fn(0, 3)(S.M(x))
    for a, b in zip(maps, want):
        assert a.dtype == np.int16 and np.array_equal(S.M(a), b)
    # a floor in the signed domain, not a truncation toward zero: the mean of seven -1 and one 0 ...
    w = np.full((1, 2, 2, 2, 1), -1, np.int16)
    w[0, 0, 0, 0, 0] = 0
    c = S.predictions(w, S.mean_fn(0, 3))[3]  # the centre map: the cell mean itself
    assert c.reshape(-1)[0] == -1  # floor(-7/8) = -1; truncation would give 0


@pytest.mark.parametrize('name,ndim', [('signed_vol_i16', 3), ('signed_img_i8', 2)])
@pytest.mark.parametrize('padding', [0, 1])
def test_golden_fixtures_match_the_spec(name, ndim, padding):
    g = load_golden(f'{name}_p{padding}')
    x = g['highres']
    assert x.dtype in (np.int8, np.int16) and x.size <= 2 * 17 ** 3
    lo, maps, dims = S.encode(x, S.mean_fn(padding, ndim), ndim, padding)
    assert np.array_equal(lo, g['lowres']) and lo.dtype == g['lowres'].dtype
    assert tuple(g['dims']) == dims
    for a, b in zip(maps, golden_maps(g, ndim)):
        assert np.array_equal(a, b) and a.dtype == b.dtype
