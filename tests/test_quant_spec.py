"""The error-bounded float32 quantiser's rule (tests/quant_spec.py), on the CPU: the exponent, known
answers, the bound on random bit patterns, the container's gap arrays and what the rule buys in size."""

import math

import numpy as np
import pytest

import quant_spec as Q

FLT_MAX = float(np.finfo(np.float32).max)


def test_exponent_around_powers_of_two():
    for k in (-126, -20, -1, 0, 1, 10, 126):
        p = math.ldexp(1.0, k)
        assert Q.exponent(p) == k + 1 and Q.effective(p) == p  # a power of two is kept as it is
        assert Q.exponent(math.nextafter(p, 0.0)) == k and Q.effective(math.nextafter(p, 0.0)) == p / 2
        assert Q.exponent(math.nextafter(p, math.inf)) == k + 1
    for a in (1e-4, 1e-3, 1e-2, 1e-1, 3.0, 1e30):
        assert a / 2 < Q.effective(a) <= a


def test_exponent_ends_of_the_range():
    assert Q.exponent(math.ldexp(1.0, -127)) == -126
    assert Q.exponent(math.ldexp(1.0, 126)) == 127
    assert Q.exponent(math.nextafter(math.ldexp(1.0, 127), 0.0)) == 127
    for bad in (math.ldexp(1.0, -128), math.nextafter(math.ldexp(1.0, -127), 0.0), math.ldexp(1.0, 127), 1e300, 1e-300):
        with pytest.raises(ValueError):
            Q.exponent(bad)
    for bad in (0, 0.0, -1.0, math.nan, math.inf, -math.inf, True, False, '1e-3', None):
        with pytest.raises(ValueError):
            Q.exponent(bad)


@pytest.mark.parametrize('dtype', [np.int16, np.int32])
@pytest.mark.parametrize('e', Q.EXPONENTS)
def test_known_answers(e, dtype):
    x, n_want, exc_want = Q.known_answers(e, dtype)
    n, exc = Q.quantise_as(x, e, dtype)
    assert np.array_equal(exc, exc_want)
    assert np.array_equal(n.astype(np.int64), n_want)
    bits = Q.encode_bits(x, e, dtype)
    assert np.all(bits[exc] == np.iinfo(dtype).min) and np.array_equal(bits[~exc], n[~exc])
    r = Q.dequant(n, e)
    assert np.all(r[~exc].view(np.uint32) != 0x80000000)  # -0.0 restores as +0.0
    idx = np.flatnonzero(exc)
    back = Q.restore(n, e, (idx, x.view(np.uint32)[idx]))
    assert np.array_equal(back.view(np.uint32)[exc], x.view(np.uint32)[exc])  # NaN payload, sign of infinities


def test_known_answers_cover_the_edges():
    for dtype in (np.int16, np.int32):
        x, n, exc = Q.known_answers(0, dtype)
        assert {0.5, 1.5, 2.5}.issubset(set(x.tolist())) and exc.sum() == 5  # NaN, +-inf, +-(QMAX + 1)
        assert int(np.abs(n).max()) == (32767 if dtype == np.int16 else 2 ** 31 - 128)
        assert float(Q.QMAX[np.dtype(dtype)] + 1) in x.tolist() and -float(Q.QMAX[np.dtype(dtype)] + 1) in x.tolist()


def test_subnormals_and_flt_max():
    sub = np.array([1e-45, -1e-45, 5.877e-39, -5.877e-39, 1.1754942e-38], np.float32)  # all subnormal
    n, exc = Q.quantise_as(sub, -126, np.int16)
    assert not exc.any() and set(n.tolist()) <= {0, 1, -1}
    assert np.abs(Q.dequant(n, -126).astype(np.float64) - sub.astype(np.float64)).max() <= math.ldexp(1.0, -127)
    n, exc = Q.quantise_as(sub, 0, np.int32)
    assert not exc.any() and not n.any()
    top = np.array([FLT_MAX, -FLT_MAX, math.ldexp(1.0, 127), 1.5 * math.ldexp(1.0, 127)], np.float32)
    n, exc = Q.quantise_as(top, 127, np.int16)  # rint(FLT_MAX / 2^127) = 2 restores to 2^128: not finite
    assert exc.tolist() == [True, True, False, True] and n.tolist() == [0, 0, 1, 0]
    n, exc = Q.quantise_as(top, 100, np.int32)  # within the int32 range there
    assert not exc.any()


@pytest.mark.parametrize('e', Q.EXPONENTS)
def test_bound_on_random_bit_patterns(e):
    x = Q.random_bits(2_000_000, seed=e & 0xff)
    eps = math.ldexp(1.0, e - 1)
    finite = np.isfinite(x)
    for dtype in (np.int16, np.int32):
        n, exc = Q.quantise_as(x, e, dtype)
        assert exc[~finite].all()
        r = Q.dequant(n, e)
        ok = ~exc
        assert np.isfinite(r[ok]).all()
        assert np.abs(r[ok].astype(np.float64) - x[ok].astype(np.float64)).max(initial=0.0) <= eps
        n2, exc2 = Q.quantise_as(r, e, dtype)  # quantise(restore(n)) == n
        assert not exc2[ok].any() and np.array_equal(n2[ok], n[ok])
        assert np.abs(n.astype(np.int64)).max() <= Q.QMAX[np.dtype(dtype)]
    if e == 100:  # 2^31 steps of 2^100 pass FLT_MAX: only what is not finite is an exception
        assert np.array_equal(Q.quantise_as(x, e, np.int32)[1], ~finite)
    if e == 127:  # finite values near FLT_MAX restore to infinity there
        assert (Q.quantise_as(x, e, np.int32)[1] & finite).any()


def test_dtype_choice_and_exceptions():
    x = np.array([[0.25, -3.0, np.nan], [100.0, np.inf, -0.0]], np.float32)
    n, exc = Q.quantise(x, -2)
    assert n.dtype == np.int16 and n.tolist() == [[1, -12, 0], [400, 0, 0]]
    assert exc[0].dtype == np.int64 and exc[0].tolist() == [2, 4] and exc[1].dtype == np.uint32
    assert np.array_equal(Q.restore(n, -2, exc).view(np.uint32), np.where(x == 0, np.float32(0), x).view(np.uint32))
    n, exc = Q.quantise(np.array([32767.0, -32767.0], np.float32), 0)
    assert n.dtype == np.int16 and exc is None
    n, exc = Q.quantise(np.array([32768.0, 1.0], np.float32), 0)
    assert n.dtype == np.int32 and exc is None and n.tolist() == [32768, 1]
    n, exc = Q.quantise(np.array([3e9, 1.0], np.float32), 0)  # out of int32: an exception, the rest fits int16
    assert n.dtype == np.int16 and exc[0].tolist() == [0]
    n, exc = Q.quantise(np.array([np.nan, np.inf], np.float32), 0)  # all exceptions
    assert n.dtype == np.int16 and not n.any() and exc[0].tolist() == [0, 1]


def test_gap_arrays_round_trip_indices_above_2_to_32():
    idx = np.array([0, 1, 5, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 7, 2 ** 33 + 2 ** 32 + 3, 2 ** 40, 2 ** 40 + 1], np.int64)
    lo, hi = Q.gaps_from_indices(idx)
    assert lo.dtype == np.uint32 and hi.dtype == np.uint32 and hi.any()
    assert np.array_equal(Q.indices_from_gaps(lo, hi), idx)
    first = np.array([2 ** 35 + 9], np.int64)  # the first gap is the first index
    assert np.array_equal(Q.indices_from_gaps(*Q.gaps_from_indices(first)), first)


def test_level_exceptions():
    shape = (2, 5, 6, 7, 1)
    idx = np.ravel_multi_index(([0, 0, 1, 1], [0, 2, 4, 4], [0, 4, 2, 4], [0, 6, 4, 4], [0, 0, 0, 0]), shape)
    bits = np.arange(4, dtype=np.uint32)
    i1, b1, s1 = Q.level_exceptions((idx, bits), shape, 3, 1)
    assert s1 == (2, 3, 3, 4, 1) and b1.tolist() == [0, 1, 2, 3]
    i2, b2, s2 = Q.level_exceptions((idx, bits), shape, 3, 2)
    assert s2 == (2, 2, 2, 2, 1) and b2.tolist() == [0, 3]
    assert i2.tolist() == [0, int(np.ravel_multi_index((1, 1, 1, 1, 0), s2))]


@pytest.fixture(scope='module')
def field_bits():
    x = Q.spec_field()
    out = {}
    for a in (1e-4, 1e-3, 1e-2, 1e-1):
        n, exc = Q.quantise(x, Q.exponent(a))
        assert exc is None and n.dtype == np.int16
        assert np.abs(Q.restore(n, Q.exponent(a), None).astype(np.float64) - x.astype(np.float64)).max() <= Q.effective(a)
        out[a] = Q.pyramid_bits(n, 3, 0, 2)
    return out


def test_size_on_the_spec_field(field_bits):
    b = field_bits
    print({a: round(v, 3) for a, v in b.items()})
    assert b[1e-4] > b[1e-3] > b[1e-2] > b[1e-1]
    assert b[1e-2] < 8.0  # the CPU oracle measured 5.51; the margin is Rice block granularity
