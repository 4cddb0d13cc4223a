"""The relative-error float32 quantiser's rule (tests/prec_spec.py), on the CPU: the kept mantissa
bits, known answers, the guarantee and idempotence on random bit patterns, the integer type, the total
decode, level exceptions and what the rule buys in size."""

import math

import numpy as np
import pytest

import prec_spec as P
import quant_spec as Q

FLT_MAX_BITS = 0x7f7fffff
MS = (0, 6, 7, 8, 22)


def f32(*bits):
    return np.array(bits, np.uint32).view(np.float32)


def test_mantissa_bits_around_powers_of_two():
    for k in range(1, 24):
        p = math.ldexp(1.0, -k)
        assert P.mantissa_bits(p) == k - 1 and P.effective_rel(p) == p  # a power of two is kept as it is
        if k > 1:
            assert P.mantissa_bits(math.nextafter(p, 1.0)) == k - 1
        if k < 23:
            assert P.mantissa_bits(math.nextafter(p, 0.0)) == k and P.effective_rel(math.nextafter(p, 0.0)) == p / 2
    for r in (0.5, 1e-1, 1e-2, 1e-3, 1e-6, 0.999, np.float32(0.25), np.float64(0.3)):
        assert r / 2 < P.effective_rel(r) <= r
    assert (P.mantissa_bits(1e-1), P.mantissa_bits(1e-2), P.mantissa_bits(1e-3)) == (3, 6, 9)


def test_mantissa_bits_ends_of_the_range():
    assert P.mantissa_bits(math.nextafter(1.0, 0.0)) == 0 and P.mantissa_bits(0.5) == 0
    assert P.mantissa_bits(math.ldexp(1.0, -23)) == 22
    for bad in (1, 1.0, 2.0, math.nextafter(math.ldexp(1.0, -23), 0.0), math.ldexp(1.0, -24), 1e-300, 1e300, 10 ** 400):
        with pytest.raises(ValueError):
            P.mantissa_bits(bad)
    for bad in (0, 0.0, -0.5, math.nan, math.inf, -math.inf, True, False, '1e-3', b'1', None, [0.5]):
        with pytest.raises(ValueError):
            P.mantissa_bits(bad)
        with pytest.raises(ValueError):
            P.effective_rel(bad)


@pytest.mark.parametrize('dtype', [np.int16, np.int32])
@pytest.mark.parametrize('m', MS)
def test_known_answers(m, dtype):
    x, n_want, exc_want = P.known_answers(m, dtype)
    n, exc = P.quantise_as(x, m, dtype)
    assert np.array_equal(exc, exc_want)
    assert np.array_equal(n.astype(np.int64), n_want)
    bits = P.encode_bits(x, m, dtype)
    assert np.all(bits[exc] == np.iinfo(dtype).min) and np.array_equal(bits[~exc], n[~exc])
    ok = ~exc
    r = P.dequant(n, m)
    assert np.isfinite(r[ok]).all()
    assert (P.rel_errors(x[ok], r[ok]) <= 2.0 ** -(m + 1)).all()
    idx = np.flatnonzero(exc)
    back = P.restore(n, m, (idx, x.view(np.uint32)[idx]))
    assert np.array_equal(back.view(np.uint32)[exc], x.view(np.uint32)[exc])  # NaN payloads and signs, bit for bit


def test_known_answers_cover_the_edges():
    for m in MS:
        for dtype in (np.int16, np.int32):
            x, n, exc = P.known_answers(m, dtype)
            u = x.view(np.uint32)
            t = 23 - m
            for bits in (0, 0x80000000, 1, 0x007fffff, 0x00800000, FLT_MAX_BITS, 0x7f800000, 0xff800000, 0x7fc12345,
                         0xffc12345, 0x3fffffff, 0x3f800000 + (1 << (t - 1))):
                assert bits in u, hex(bits)
            assert not n[u == 0x80000000].any() and not exc[u == 0x80000000].any()  # -0.0 gives 0
            assert exc[u == FLT_MAX_BITS].all() and exc[(u & 0x7fffffff) >= 0x7f800000].all()
            ktop = 255 * 2 ** m - 1
            assert int(np.abs(n).max()) == min(ktop, P.QMAX[np.dtype(dtype)])
            assert (exc & ((u & 0x7fffffff) < 0x7f800000)).any()  # a finite value that is an exception


def test_literal_answers():
    # m = 7, t = 16: 1.0 is 0x3f80 << 16
    x = f32(0x3f800000, 0xbf800000, 0x3f808000, 0x3f818000, 0x3f807fff, 0x3fffffff, 0x7f7f7fff, 0x7f7f8000)
    n, exc = P.quantise_as(x, 7, np.int16)
    assert n.tolist() == [0x3f80, -0x3f80, 0x3f80, 0x3f82, 0x3f80, 0x4000, 0x7f7f, 0]
    assert exc.tolist() == [False] * 7 + [True]
    assert P.dequant(n[:7], 7).view(np.uint32).tolist() == [0x3f800000, 0xbf800000, 0x3f800000, 0x3f820000, 0x3f800000,
                                                            0x40000000, 0x7f7f0000]
    # m = 8, t = 15: k of 2.0 is 0x8000, the first above int16; the tie below it rounds up to it
    x = f32(0x40000000, 0x3fffc000, 0x3fffbfff, 0xc0000000)
    n16, exc16 = P.quantise_as(x, 8, np.int16)
    n32, exc32 = P.quantise_as(x, 8, np.int32)
    assert exc16.tolist() == [True, True, False, True] and n16.tolist() == [0, 0, 32767, 0]
    assert not exc32.any() and n32.tolist() == [32768, 32768, 32767, -32768]
    # m = 0: only the sign and the exponent survive; 1.5 is a tie and goes to the even 2.0
    x = f32(0x3f800000, 0x3fc00000, 0x3fbfffff, 0x40400000, 0x00400000, 0x00400001)
    n, exc = P.quantise_as(x, 0, np.int16)
    assert n.tolist() == [127, 128, 127, 128, 0, 1] and not exc.any()
    # m = 22, t = 1: FLT_MAX itself is a tie that rounds up to infinity, the value below it stays
    n, exc = P.quantise_as(f32(0x7f7ffffe, 0x7f7fffff, 0x00000001, 0x00000003), 22, np.int32)
    assert exc.tolist() == [False, True, False, False] and n.tolist() == [0x3fbfffff, 0, 0, 2]


@pytest.mark.parametrize('m', P.BITS)
def test_guarantee_and_idempotence_on_random_bit_patterns(m):
    x = P.random_bits(1_000_000, seed=m)
    eps = 2.0 ** -(m + 1)
    finite = np.isfinite(x)
    worst = {}
    for dtype in (np.int16, np.int32):
        n, exc = P.quantise_as(x, m, dtype)
        assert exc[~finite].all()
        ok = ~exc
        r = P.dequant(n, m)
        assert np.isfinite(r[ok]).all()
        worst[dtype] = float(P.rel_errors(x[ok], r[ok]).max(initial=0.0))
        assert worst[dtype] <= eps
        n2, exc2 = P.quantise_as(r, m, dtype)  # quantise(restore(n)) == n
        assert not exc2[ok].any() and np.array_equal(n2[ok], n[ok])
        assert np.abs(n.astype(np.int64)).max() <= min(P.QMAX[np.dtype(dtype)], 255 * 2 ** m - 1)
        assert np.array_equal(np.signbit(x[ok])[n[ok] != 0], (n[ok] < 0)[n[ok] != 0])
    print(m, {np.dtype(k).name: v / eps for k, v in worst.items()})
    n32, exc32 = P.quantise_as(x, m, np.int32)
    if m <= 7:  # a million patterns reach the top code (about 2^(12-m) of them fall in its cell)
        assert int(np.abs(n32.astype(np.int64)).max()) == 255 * 2 ** m - 1
    # the int32 exceptions: what is not finite plus the few that round to infinity -- the top half of
    # the last code's cell, 2^(22-m) of the 2^31 magnitudes; twice the expected count, plus ten
    assert (exc32 & finite).sum() <= x.size * 2.0 ** -(8 + m) + 10
    # n is monotone in x over the non-exceptions
    o = np.argsort(x[~exc32], kind='stable')
    assert (np.diff(n32[~exc32][o].astype(np.int64)) >= 0).all()


def test_dtype_choice_and_equal_exception_sets():
    for m in range(0, 8):  # 255 * 2^7 - 1 = 32639: int16 whatever the data
        x = P.random_bits(50_000, seed=100 + m)
        n, exc = P.quantise(x, m)
        assert n.dtype == np.int16
        assert np.array_equal(P.quantise_as(x, m, np.int16)[1], P.quantise_as(x, m, np.int32)[1])
    small = np.array([[0.25, -1.99, np.nan], [1e-30, np.inf, -0.0]], np.float32)
    n, exc = P.quantise(small, 8)  # every |x| < 2.0 at m = 8: k <= 32767
    assert n.dtype == np.int16 and exc[0].dtype == np.int64 and exc[0].tolist() == [2, 4] and exc[1].dtype == np.uint32
    assert exc[1].tolist() == [0x7fc00000, 0x7f800000] and n.reshape(-1)[exc[0]].tolist() == [0, 0]
    back = P.restore(n, 8, exc)
    assert back.shape == small.shape and np.array_equal(back.view(np.uint32)[0, 2], small.view(np.uint32)[0, 2])
    assert back.view(np.uint32)[1, 2] == 0  # -0.0 restores as +0.0
    n, exc = P.quantise(np.array([2.0, 0.5], np.float32), 8)
    assert n.dtype == np.int32 and exc is None and n.tolist() == [32768, 32256]
    n, exc = P.quantise(np.array([np.nan, -np.inf], np.float32), 22)  # all exceptions
    assert n.dtype == np.int16 and not n.any() and exc[0].tolist() == [0, 1]
    n, exc = P.quantise(np.zeros((0, 3), np.float32), 10)
    assert n.dtype == np.int16 and n.shape == (0, 3) and exc is None


def test_decode_is_total():
    for m in MS:
        t = 23 - m
        for dtype, top in ((np.int16, 15), (np.int32, 31)):
            info = np.iinfo(dtype)
            n = np.array([info.min, -1, 0, 1, info.max], dtype)
            want = [((1 << top << t) & 0x7fffffff) | 0x80000000, (1 << t) | 0x80000000, 0, 1 << t,
                    (info.max << t) & 0x7fffffff]
            assert P.dequant(n, m).view(np.uint32).tolist() == want, (m, dtype)
        allv = np.arange(-32768, 32768).astype(np.int16)
        assert P.dequant(allv, m).shape == allv.shape


def test_level_exceptions():
    shape = (2, 5, 6, 7, 1)
    x = np.ones(shape, np.float32)
    at = ([0, 0, 1, 1], [0, 2, 4, 4], [0, 4, 2, 4], [0, 6, 4, 4], [0, 0, 0, 0])
    x[at] = [np.nan, np.inf, -np.inf, 3.4028235e38]
    n, exc = P.quantise(x, 6)
    assert exc[0].tolist() == np.ravel_multi_index(at, shape).tolist()
    full = P.restore(n, 6, exc)
    for k, kept in ((1, 4), (2, 2)):
        idx, bits, lshape = Q.level_exceptions(exc, shape, 3, k)
        assert idx.size == kept
        top = P.restore(np.ascontiguousarray(n[:, ::2 ** k, ::2 ** k, ::2 ** k]), 6, (idx, bits))
        assert top.shape == lshape
        assert np.array_equal(top.view(np.uint32), np.ascontiguousarray(full[:, ::2 ** k, ::2 ** k, ::2 ** k]).view(np.uint32))


@pytest.fixture(scope='module')
def field_bits():
    x = P.decades_field()
    out = {}
    for m in (3, 5, 7):
        n, exc = P.quantise(x, m)
        assert exc is None and n.dtype == np.int16
        assert P.rel_errors(x, P.restore(n, m, None)).max() <= 2.0 ** -(m + 1)
        out[m] = Q.pyramid_bits(n, 3, 0, 2)
    return out


def test_size_on_the_decades_field(field_bits):
    """Four decades, 5 % multiplicative noise, [1, 40, 48, 56, 1], MeanPredictor(0), 2 levels: 4.60 / 6.49 /
    8.49 Rice bits per sample at m = 3 / 5 / 7 -- two bits per two mantissa bits, as noise-dominated data must."""
    b = field_bits
    print({m: round(v, 3) for m, v in b.items()})
    assert b[3] < b[5] < b[7] < 16.0
