"""The time-series specification (tests/delta_spec.py) against numpy and the oracle alone: no GPU, no product."""

import numpy as np
import pytest

import delta_spec as D
import signed_spec as S

KS = (None, 1, 2, 3, 'T')
IDS = [np.dtype(d).name for d in D.DTYPES]


def uniform(shape, dtype, seed):
    info = np.iinfo(dtype)
    return np.random.default_rng(seed).integers(info.min, int(info.max) + 1, size=shape, dtype=np.int64).astype(dtype)


@pytest.mark.parametrize('dtype', D.DTYPES, ids=IDS)
def test_round_trip(dtype):
    for T in (1, 2, 5):
        n = uniform((T, 3, 4, 5, 1), dtype, seed=T)
        n.reshape(-1)[:2] = np.iinfo(dtype).min, np.iinfo(dtype).max
        for K in KS:
            K = T if K == 'T' else K
            d = D.encode(n, K)
            assert d.dtype == D.SIGNED[np.dtype(dtype)] and d.shape == n.shape
            back = D.decode(d, dtype, K)
            assert back.dtype == np.dtype(dtype) and np.array_equal(back, n), (T, K)
            for t in range(T):  # the rule, frame by frame, in Python integers
                if D.is_key(t, K):
                    assert np.array_equal(d[t].view(dtype), n[t])
                else:
                    W = 8 * np.dtype(dtype).itemsize
                    want = (n[t].astype(np.int64) - n[t - 1].astype(np.int64)) % (1 << W)
                    assert np.array_equal(d[t].astype(np.int64) % (1 << W), want)
            if T == 1 or K == 1:  # key frames alone: the samples' own bits
                assert np.array_equal(d.view(dtype), n)


def test_key_frames():
    assert [t for t in range(7) if D.is_key(t, None)] == [0]
    assert [t for t in range(7) if D.is_key(t, 1)] == list(range(7))
    assert [t for t in range(7) if D.is_key(t, 3)] == [0, 3, 6]
    assert [t for t in range(7) if D.is_key(t, 7)] == [0]
    for bad in (True, False, 0, -1, 2.0, '2'):
        with pytest.raises(ValueError):
            D.check_key_interval(bad)
    assert D.frames_read(3, 4, 2) == (2, 4) and D.frames_read(3, 4, None) == (0, 4) and D.frames_read(4, 5, 2) == (4, 5)


def test_wraps():
    n = np.array([0, 65535, 0], np.uint16).reshape(3, 1)
    d = D.encode(n)
    assert d.dtype == np.int16 and d.reshape(-1).tolist() == [0, -1, 1]  # small signed values, not 65535
    assert np.array_equal(D.decode(d, np.uint16), n)
    n = np.array([-32768, 32767, -32768], np.int16).reshape(3, 1)
    d = D.encode(n)
    assert d.reshape(-1).tolist() == [-32768, -1, 1] and np.array_equal(D.decode(d, np.int16), n)
    n = np.array([0, 255, 0], np.uint8).reshape(3, 1)
    d = D.encode(n)
    assert d.dtype == np.int8 and d.reshape(-1).tolist() == [0, -1, 1] and np.array_equal(D.decode(d, np.uint8), n)
    # a key frame of unsigned samples is reinterpreted bit for bit
    n = np.array([200, 201], np.uint8).reshape(2, 1)
    assert D.encode(n, 1).reshape(-1).tolist() == [-56, -55] and D.encode(n).reshape(-1).tolist() == [-56, 1]


@pytest.mark.parametrize('K', (None, 2))
def test_levels_commute(K):
    n = uniform((5, 9, 10, 13, 1), np.int16, seed=4)
    d = D.encode(n, K)
    for k in (1, 2):
        assert np.array_equal(D.level(d, 3, k), D.encode(D.level(n, 3, k), K))
    # ... and the codec's own lowres is that level: the pyramid of d holds the deltas of the pyramid of n
    fn = S.mean_fn(0, 3)
    xn, xd = n, d
    for k in (1, 2):
        xn, xd = S.encode(xn, fn, 3, 0)[0], S.encode(xd, fn, 3, 0)[0]
        assert np.array_equal(xn, D.level(n, 3, k)) and np.array_equal(xd, D.encode(xn, K))


def test_size_on_the_spec_sequence():
    """The table of DESIGN.md §22 (seed ``delta_spec.SEED``): delta is smaller than independent in every row."""
    rows = []
    for shift, noise in D.ROWS:
        for e in D.EXPONENTS:
            ind, dlt = D.size_row(shift, noise, e)
            rows.append((shift, noise, e, ind, dlt))
            print(f'shift {shift:<5} noise {noise:<7.4f} e {e:>3}: independent {ind:6.2f}  delta {dlt:6.2f} bits per sample')
    for shift, noise, e, ind, dlt in rows:
        assert dlt < ind, (shift, noise, e, ind, dlt)
