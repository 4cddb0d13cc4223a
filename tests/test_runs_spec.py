"""The rule of masked float32 fields (tests/runs_spec.py) against itself: runs <-> exceptions,
known answers of the fill, and the size table the design quotes."""

import numpy as np
import pytest

import quant_spec
import runs_spec
import signed_spec

U = np.uint32
NAN, NAN2, PINF = 0x7fc00000, 0x7fc00001, 0x7f800000


def exc(idx, bits):
    return np.array(idx, np.int64), np.array(bits, np.uint32)


CASES = {
    'empty': (exc([], []), 0),
    'one': (exc([5], [NAN]), 1),
    'adjacent, different bits': (exc([7, 8], [NAN, PINF]), 2),
    'equal bits, one index apart': (exc([7, 9], [NAN, NAN]), 2),
    'a stretch': (exc([3, 4, 5, 6], [NAN] * 4), 1),
    'a stretch cut by its bits': (exc([3, 4, 5, 6], [NAN, NAN, NAN2, NAN2]), 2),
    'above 2**32': (exc([1, 2 ** 32 + 5, 2 ** 32 + 6, 2 ** 40], [NAN, PINF, PINF, 0xffffffff]), 3),
}


@pytest.mark.parametrize('name', list(CASES))
def test_round_trip(name):
    (idx, bits), R = CASES[name]
    stored = runs_spec.runs((idx, bits))
    assert all(a.dtype == U and a.shape == (R,) for a in stored)
    back = runs_spec.exceptions_from_runs(*stored)
    assert back[0].dtype == np.int64 and back[1].dtype == U
    assert np.array_equal(back[0], idx) and np.array_equal(back[1], bits)


def test_stored_form():
    lo, hi, lengths, delta = runs_spec.runs(exc([2 ** 32 + 5, 2 ** 32 + 6, 2 ** 33], [PINF, PINF, NAN]))
    assert lo.tolist() == [5, 2 ** 32 - 5] and hi.tolist() == [1, 0] and lengths.tolist() == [2, 1]
    assert delta.tolist() == [PINF, NAN - PINF]
    # a falling bit pattern wraps modulo 2**32
    assert runs_spec.runs(exc([0, 1], [NAN, PINF]))[3].tolist() == [NAN, (PINF - NAN) % 2 ** 32]


@pytest.mark.parametrize('cap', [1, 3, 4, 5])
def test_run_cap(cap):
    idx, bits = exc([*range(10, 20), 30], [NAN] * 11)
    starts, lengths, rbits = runs_spec.runs_from_exceptions(idx, bits, cap=cap)
    assert lengths.max() <= cap and lengths.min() >= 1 and lengths.sum() == 11
    assert len(starts) == -(-10 // cap) + 1 and starts[0] == 10 and starts[-1] == 30
    back = runs_spec.exceptions_from_runs(*runs_spec.runs((idx, bits), cap=cap))
    assert np.array_equal(back[0], idx) and np.array_equal(back[1], bits)


@pytest.mark.parametrize('dtype', [np.int16, np.int32])
def test_fill_known_answers(dtype):
    M = runs_spec.mark(dtype)
    rows = {'leading': ([M, M, 4, 5], [4, 4, 4, 5]), 'trailing': ([4, -5, M, M], [4, -5, -5, -5]),
            'all': ([M, M, M], [0, 0, 0]), 'none': ([1, -2, 3], [1, -2, 3]),
            'alternating': ([M, 1, M, 2, M, -3, M], [1, 1, 1, 2, 2, -3, -3]), 'empty': ([], [])}
    for name, (marked, want) in rows.items():
        marked = np.array(marked, dtype)
        got = runs_spec.fill(marked)
        assert got.dtype == marked.dtype and got.tolist() == want, name
        ok = marked != M
        assert runs_spec.extent(got, np.ones(got.shape, bool)) == runs_spec.extent(marked, ok), name
    x = np.array([[M, 7], [M, M]], dtype)
    assert runs_spec.fill(x).tolist() == [[7, 7], [7, 7]]  # flat C order, the shape kept


def test_fill_keeps_the_integer_dtype_choice():
    x = quant_spec.spec_field()
    x[0, 3:5] = np.nan
    n, e = quant_spec.quantise(x, -6)
    filled = runs_spec.fill(runs_spec.marked(n, e))
    assert filled.dtype == n.dtype
    ok = np.ones(n.size, bool)
    ok[e[0]] = False
    assert runs_spec.extent(filled, np.ones(n.shape, bool)) == runs_spec.extent(n.reshape(-1), ok)
    assert np.array_equal(filled.reshape(-1)[ok], n.reshape(-1)[ok])


# ---- the size table of DESIGN.md §21 -------------------------------------------------------------------

def _masks():
    shape = (40, 48, 56)
    z, y, x = np.meshgrid(*[np.arange(s) for s in shape], indexing='ij')
    size = int(np.prod(shape))
    slab = np.zeros(shape, bool)
    slab[16:20] = True  # planes 16:20 of batch item 0
    ell = ((z - 20) ** 2 / 400 + (y - 24) ** 2 / 500 + (x - 28) ** 2 / 500) < 0.62
    scattered = np.zeros(size, bool)
    scattered[np.random.default_rng(3).choice(size, size // 100, replace=False)] = True
    inf = np.zeros(size, bool)
    inf[np.random.default_rng(3).choice(size, size // 200, replace=False)] = True
    nan = np.float32(np.nan)
    return [('slab', -6, [(slab, nan)]), ('slab', -3, [(slab, nan)]), ('ellipsoid', -6, [(ell, nan)]),
            ('ellipsoid', -3, [(ell, nan)]), ('scattered', -6, [(scattered.reshape(shape), nan)]),
            ('slab + inf', -6, [(slab, nan), (inf.reshape(shape), np.float32(np.inf))])]


def _bits(arrays, size):
    return signed_spec.rice_bits_per_sample(arrays) * sum(a.size for a in arrays) / size if arrays else 0.0


def _maps_bits(n):
    return quant_spec.pyramid_bits(n, 3, 0, 2)


@pytest.fixture(scope='module')
def table():
    field = quant_spec.spec_field()
    clean = {e: _maps_bits(quant_spec.quantise(field, e)[0]) for e in (-6, -3)}
    rows = []
    for name, e, masks in _masks():
        x = field.copy()
        for m, v in masks:
            x[0, ..., 0][m] = v
        n, ex = quant_spec.quantise(x, e)
        lo, hi = quant_spec.gaps_from_indices(ex[0])
        today = (_maps_bits(n), _bits([lo, hi, ex[1]], x.size))
        stored = runs_spec.runs(ex)
        new = (_maps_bits(runs_spec.fill(runs_spec.marked(n, ex))), _bits(list(stored), x.size))
        rows.append({'mask': name, 'e': e, 'E': ex[0].size, 'R': stored[0].size, 'today': today, 'runs': new,
                     'clean': clean[e]})
        print(f'{name:12s} e={e:3d} E={ex[0].size:6d} R={stored[0].size:5d}  today {today[0]:.3f} + {today[1]:.3f} = '
              f'{sum(today):.3f}   runs + fill {new[0]:.3f} + {new[1]:.3f} = {sum(new):.3f}   clean {clean[e]:.3f}')
    return rows


def test_size_table_runs_and_fill_are_smaller(table):
    assert len(table) == 6
    for r in table:
        assert sum(r['runs']) < sum(r['today']), r


def test_size_table_slabs_close_to_the_clean_field(table):
    slabs = [r for r in table if r['mask'] == 'slab']
    assert len(slabs) == 2
    for r in slabs:
        assert sum(r['runs']) <= r['clean'] + 0.05, r


def test_size_table_run_arrays_are_cheap(table):
    for r in table:
        assert r['runs'][1] < 0.2, r
