"""The near-lossless rule (tests/near_spec.py) checked against its own consequences, from numpy and
the oracle alone: the bound, the width of q, the closed loop's level consistency and the Rice saving
the quantiser buys on a noisy field."""

import numpy as np
import pytest

import near_spec as NS
from signed_spec import M


@pytest.mark.parametrize('delta', NS.U8_DELTAS)
def test_uint8_every_pair(delta):
    pred, x = NS.pair_table(np.uint8, delta)
    P, X = pred.astype(np.int64), x.astype(np.int64)
    enc = NS.encode_values(pred, x, delta)
    assert enc.dtype == np.uint8
    q = NS.signed_q(enc)
    assert np.array_equal(q, NS.quantise(P, X, delta))          # nothing wrapped in the W-bit store
    assert np.abs(q).max() <= (255 + delta) // (2 * delta + 1) < 128  # W - 1 bits plus sign
    R, raw = NS.reconstruct(P, q, delta, 8)
    assert np.abs(raw - X).max() <= delta                        # before the clamp
    dec = NS.decode_values(pred, enc, delta, np.uint8)
    assert dec.dtype == np.uint8 and np.array_equal(dec.astype(np.int64), R)
    assert np.abs(dec.astype(np.int64) - X).max() <= delta


@pytest.mark.parametrize('delta', NS.U16_DELTAS)
def test_uint16_boundary_predictions(delta):
    pred, x = NS.pair_table(np.uint16, delta)
    P, X = pred.astype(np.int64), x.astype(np.int64)
    assert set(np.unique(P)) == set(NS.u16_predictions(delta).tolist())
    enc = NS.encode_values(pred, x, delta)
    q = NS.signed_q(enc)
    assert np.array_equal(q, NS.quantise(P, X, delta))
    assert np.abs(q).max() <= (65535 + delta) // (2 * delta + 1) < 32768
    _, raw = NS.reconstruct(P, q, delta, 16)
    assert np.abs(raw - X).max() <= delta
    dec = NS.decode_values(pred, enc, delta, np.uint16)
    assert np.abs(dec.astype(np.int64) - X).max() <= delta


@pytest.mark.parametrize('dtype,delta', [(np.int8, 1), (np.int8, 7), (np.int8, 127), (np.int16, 2), (np.int16, 255),
                                         (np.int16, 32767)])
def test_signed_is_the_unsigned_rule_on_M(dtype, delta):
    pred, x = NS.pair_table(dtype, delta)
    enc = NS.encode_values(pred, x, delta)
    assert np.array_equal(enc, NS.encode_values(M(pred), M(x), delta))
    dec = NS.decode_values(pred, enc, delta, dtype)
    assert dec.dtype == np.dtype(dtype)
    assert np.array_equal(M(dec), NS.decode_values(M(pred), enc, delta, NS.map_dtype(dtype)))
    # equivalently: the clamp is the signed type's own range
    assert np.abs(dec.astype(np.int64) - x.astype(np.int64)).max() <= delta


@pytest.mark.parametrize('dtype', NS.DTYPES)
def test_float32_predictions_truncate_then_clamp(dtype):
    info = np.iinfo(dtype)
    v = NS.f32_predictions(64, dtype)
    P = NS.pred_int(v, dtype)
    assert P.min() >= 0 and P.max() <= 2 ** NS.width(dtype) - 1
    assert P[0] == 0 - int(info.min)                                  # NaN -> 0
    assert P[1] == int(info.max) - int(info.min) and P[2] == 0        # +inf / -inf saturate
    assert P[9] == P[10] == 0 - int(info.min)                         # -0.75, 0.75 truncate toward zero
    x = NS.noise((1, 64, 1), dtype, 3).reshape(-1)
    for delta in (1, NS.max_delta(dtype)):
        dec = NS.decode_values(v, NS.encode_values(v, x, delta), delta, dtype)
        assert np.abs(dec.astype(np.int64) - x.astype(np.int64)).max() <= delta


def test_argument_errors():
    with pytest.raises(TypeError):
        NS.check(np.int32, 1)
    with pytest.raises(TypeError):
        NS.check(np.float32, 1)
    for bad in (0, -1, 128, True, 1.0, None):
        with pytest.raises(ValueError):
            NS.check(np.uint8, bad)
    NS.check(np.uint8, 127)
    NS.check(np.int16, 32767)


def _predictor(kind, padding, ndim, dtype):
    if kind == 'mean':
        return NS.mean_fn(padding, ndim, dtype)
    w, b = NS.linear_weights(padding, ndim)
    return NS.linear_fn(padding, w, b, ndim, dtype)


@pytest.mark.parametrize('kind', ['mean', 'linear'])
@pytest.mark.parametrize('padding', [0, 1])
@pytest.mark.parametrize('shape,ndim', [((2, 9, 10, 11, 1), 3), ((2, 13, 10, 1), 2)])
@pytest.mark.parametrize('dtype', [np.uint8, np.uint16, np.int16])
def test_closed_loop_on_full_range_noise(dtype, shape, ndim, padding, kind):
    x = NS.noise(shape, dtype, seed=11)
    fn = _predictor(kind, padding, ndim, dtype)
    for levels in (1, 2, 3):
        for delta in (1, NS.max_delta(dtype)) if levels == 2 else (3,):
            lo, enc, r = NS.encode_pyramid(x, fn, ndim, padding, levels, delta)
            assert np.abs(r[0].astype(np.int64) - x.astype(np.int64)).max() <= delta
            for k in range(levels + 1):
                assert np.array_equal(NS.strided(r[0], ndim, k), r[k])
            assert np.array_equal(lo, NS.strided(x, ndim, levels))   # r_L is stored exactly
            assert np.array_equal(NS.decode_pyramid(lo, enc, fn, ndim, padding, delta), r[0])


def test_rice_size_falls_with_delta():
    """On the smooth-plus-noise field (noise sigma about 20) the theory's saving is log2(2 delta + 1)
    bits for a noise-dominated residual: 1.58 at delta = 1, 3.17 at delta = 4.  The bounds asked here
    are 1.0 and 2.5."""
    x = NS.noisy_field((1, 40, 48, 56, 1), np.uint16, seed=0)
    fn = NS.mean_fn(0, 3, np.uint16)
    from oracle import common as OC
    lo0, enc0 = x, []
    for _ in range(2):  # delta = 0: the modular coder, the open loop
        lo0, e = NS.ons(3).encode(fn, OC.encode_values_uint16, lo0, padding=0)
        enc0.append(e)
    b0 = NS.rice_bits(enc0, lo0)
    bits = {}
    for delta in (1, 4):
        lo, enc, r = NS.encode_pyramid(x, fn, 3, 0, 2, delta)
        assert np.abs(r[0].astype(np.int64) - x.astype(np.int64)).max() == delta
        bits[delta] = NS.rice_bits(enc, lo)
    print(f'rice bits per sample: delta 0 {b0:.3f}, 1 {bits[1]:.3f}, 4 {bits[4]:.3f}')
    assert b0 - bits[1] >= 1.0
    assert b0 - bits[4] >= 2.5
