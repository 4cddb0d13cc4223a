"""tests/metrics_spec.py against known answers, and the facts DESIGN.md §20 quotes on the spec field: the
PSNR of the 'abs' ladder falls strictly, follows the uniform-noise model in its middle, and the quality
search lands on the rungs the container tests expect."""

import math

import numpy as np
import pytest

import metrics_spec as M
import quant_spec as Q

INF, NAN = math.inf, math.nan


def test_known_answers_float():
    x = np.array([1.0, 2.0, -3.0, 0.5], np.float32)
    r = np.array([1.5, 2.0, -2.0, 0.25], np.float32)
    rec = M.record(x, r)
    assert rec == {'count': 4, 'mismatch': 0, 'max_abs': 1.0, 'sse': 0.25 + 1.0 + 0.0625, 'x_min': -3.0, 'x_max': 2.0}
    d = M.derive(rec, np.float32)
    assert d['mse'] == 1.3125 / 4 and d['rmse'] == math.sqrt(1.3125 / 4)
    assert d['value_range'] == d['peak'] == 5.0
    assert d['psnr'] == 10 * math.log10(25.0 / (1.3125 / 4)) and d['nrmse'] == d['rmse'] / 5.0
    assert M.derive(rec, np.float32, peak=10)['psnr'] == 10 * math.log10(100.0 / (1.3125 / 4))
    w = M.words(rec, True)
    assert w.dtype == np.uint64 and w.shape == (8,) and w[6] == w[7] == 0
    assert w[2] == np.array([1.0]).view(np.uint64)[0] and M.from_words(w, True) == rec


@pytest.mark.parametrize('dtype', [np.uint8, np.uint16, np.int8, np.int16])
def test_known_answers_integer(dtype):
    info = np.iinfo(dtype)
    x = np.array([info.min, info.max, 0, 7], dtype)
    r = np.array([info.max, info.min, 1, 7], dtype)
    rec = M.record(x, r)
    span = int(info.max) - int(info.min)
    assert rec == {'count': 4, 'mismatch': 0, 'max_abs': float(span), 'sse': 2 * span * span + 1,
                   'x_min': float(info.min), 'x_max': float(info.max)}
    assert isinstance(rec['sse'], int)
    d = M.derive(rec, dtype)
    assert d['peak'] == 2 ** (8 * np.dtype(dtype).itemsize) - 1 == span
    assert d['psnr'] == 10 * math.log10(span * span / ((2 * span * span + 1) / 4))
    assert int(M.words(rec, False)[3]) == 2 * span * span + 1


def test_equal_arrays():
    for x in (Q.spec_field(), np.arange(200, dtype=np.uint8), np.arange(-100, 100, dtype=np.int16)):
        d = M.compare(x, x.copy())
        assert d['count'] == x.size and d['mismatch'] == 0 and d['max_abs_error'] == 0 and d['mse'] == 0
        assert d['psnr'] == INF and d['nrmse'] == 0


def test_non_finite_values_kept_and_not_kept():
    x = np.array([1.0, NAN, INF, -INF, 2.0, NAN, 3.0, INF], np.float32)
    r = x.copy()
    assert M.record(x, r) == {'count': 3, 'mismatch': 0, 'max_abs': 0.0, 'sse': 0.0, 'x_min': 1.0, 'x_max': 3.0}
    r.view(np.uint32)[1] ^= 1   # another NaN payload
    r[2] = -INF                 # the other infinity
    r[3] = 5.0                  # an infinity restored as a number
    r[6] = NAN                  # a number restored as a NaN: not compared, a mismatch
    r[0] = 1.5
    rec = M.record(x, r)
    assert rec == {'count': 2, 'mismatch': 4, 'max_abs': 0.5, 'sse': 0.25, 'x_min': 1.0, 'x_max': 2.0}


def test_constant_field_and_zero_signs():
    x = np.full(10, 4.0, np.float32)
    d = M.compare(x, x + np.float32(0.5))
    assert d['value_range'] == d['peak'] == 0 and d['psnr'] == -INF and d['nrmse'] == INF and d['mse'] == 0.25
    assert M.compare(x, x)['psnr'] == INF and M.compare(x, x)['nrmse'] == 0
    assert M.compare(x, x + np.float32(0.5), peak=4.0)['psnr'] == 10 * math.log10(16 / 0.25)
    z = np.array([-0.0, -0.0], np.float32)
    w = M.words(M.record(z, z), True)
    assert w[4] == 0 and w[5] == 0  # a zero is +0.0 in the record


def test_nothing_compared():
    x = np.array([NAN, INF], np.float32)
    for a, b in ((x, x), (np.zeros(0, np.float32), np.zeros(0, np.float32)), (np.zeros(0, np.uint8), np.zeros(0, np.uint8))):
        rec = M.record(a, b)
        assert rec == {'count': 0, 'mismatch': 0, 'max_abs': 0.0, 'sse': 0, 'x_min': INF, 'x_max': -INF}
        d = M.derive(rec, a.dtype)
        assert d['mse'] == 0 and d['rmse'] == 0 and d['value_range'] == 0 and d['psnr'] == INF
    assert M.derive(M.record(x, x), np.float32)['peak'] == 0 and M.derive(M.record(x, x), np.float32)['nrmse'] == 0


def test_fold_is_the_record_of_the_concatenation():
    rng = np.random.default_rng(3)
    x = rng.integers(0, 65536, 1000).astype(np.uint16)
    r = rng.integers(0, 65536, 1000).astype(np.uint16)
    assert M.fold(M.fold(M.record(x[:100], r[:100]), M.record(x[100:101], r[100:101])),
                  M.record(x[101:], r[101:])) == M.record(x, r)


@pytest.fixture(scope='module')
def ladder_psnr():
    f = Q.spec_field()
    out = {}
    for e in range(-29, 3):
        n, exc = Q.quantise(f, e)
        out[e] = M.compare(f, Q.restore(n, e, exc))
    return f, out


def test_the_abs_ladder_on_the_spec_field(ladder_psnr):
    f, q = ladder_psnr
    psnr = [q[e]['psnr'] for e in range(-29, 3)]
    assert all(a > b for a, b in zip(psnr, psnr[1:]))  # strictly decreasing: monotone
    assert abs(psnr[0] - 206.7) < 0.05 and abs(psnr[-1] - 15.69) < 0.005
    rng = float(f.max()) - float(f.min())
    assert all(q[e]['peak'] == rng and q[e]['mismatch'] == 0 and q[e]['count'] == f.size for e in q)
    for e in range(-21, -1):  # the uniform-noise model: an error uniform in a step of 2^e
        assert abs(q[e]['psnr'] - 10 * math.log10(rng * rng / (4.0 ** e / 12))) < 0.1
    assert abs(q[-7]['psnr'] - 60.09) < 0.005 and abs(q[-6]['psnr'] - 54.10) < 0.005
    assert abs(q[-12]['psnr'] - 90.20) < 0.005


def test_the_spec_search_on_the_spec_field(ladder_psnr):
    _, q = ladder_psnr
    ladder = list(range(-29, 3))
    for target, e in ((60, -7), (90, -12)):
        rung, probes = M.search_quality(lambda k: q[ladder[k]]['psnr'], len(ladder), target)
        assert ladder[rung] == e and len(probes) <= 2 + math.ceil(math.log2(len(ladder)))
    with pytest.raises(M.Unreachable):
        M.search_quality(lambda k: q[ladder[k]]['psnr'], len(ladder), 1000)
