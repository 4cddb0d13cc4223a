"""The rate-control search (tests/rate_spec.py) on its own: the three guarantees -- the chosen rung fits,
the next finer one does not, at most 2 + ceil(log2 L) probes -- on monotone and on deliberately
non-monotone size functions; the product's ``rate.search`` makes the same probes.  No GPU."""

import math

import numpy as np
import pytest

import rate_spec as R

LENGTHS = [1, 2, 3, 4, 5, 7, 8, 9, 23, 32, 33, 128, 32768]


def monotone(L, seed):
    rng = np.random.default_rng(seed)
    return np.sort(rng.integers(10, 10_000, size=L))[::-1].tolist()  # rung 0 the largest


def bumpy(L, seed):
    """Sizes that fall overall but go up again here and there, with plateaus."""
    rng = np.random.default_rng(seed)
    s = np.array(monotone(L, seed)) + rng.integers(-800, 801, size=L)
    s[rng.integers(0, L, size=max(L // 4, 1))] += 3000
    return np.maximum(s, 1).tolist()


def guarantees(sizes, budget, rung, probes):
    L = len(sizes)
    assert 0 <= rung < L and sizes[rung] <= budget, 'the chosen rung fits'
    assert rung == 0 or sizes[rung - 1] > budget, 'the next finer rung does not'
    assert len(probes) <= R.max_probes(L)
    assert all(s == sizes[r] for r, s in probes) and len({r for r, _ in probes}) == len(probes)
    assert rung in {r for r, _ in probes}, 'the chosen rung was sized'


def budgets(sizes):
    out = set()
    for s in (sizes if len(sizes) <= 40 else sizes[:5] + sizes[-5:] + sizes[len(sizes) // 2 - 3:len(sizes) // 2 + 3]):
        out |= {s, s - 1, s + 1}
    out |= {(a + b) // 2 for a, b in zip(sizes[:40], sizes[1:41])}
    return sorted(out)


@pytest.mark.parametrize('make', [monotone, bumpy], ids=['monotone', 'non-monotone'])
@pytest.mark.parametrize('L', LENGTHS)
def test_the_three_guarantees(make, L):
    from kompressor_amd import rate
    for seed in range(3):
        sizes = make(L, seed)
        for budget in budgets(sizes):
            reachable = sizes[0] <= budget or sizes[-1] <= budget
            if not reachable:
                with pytest.raises(ValueError):
                    R.search(lambda r: sizes[r], L, budget)
                with pytest.raises(ValueError) as e:
                    rate.search(lambda r: sizes[r], L, budget)
                assert str(sizes[-1]) in str(e.value)  # the message names the coarsest size
                continue
            rung, probes = R.search(lambda r: sizes[r], L, budget)
            guarantees(sizes, budget, rung, probes)
            assert rate.search(lambda r: sizes[r], L, budget) == (rung, probes)


@pytest.mark.parametrize('L', LENGTHS)
def test_monotone_sizes_give_the_finest_rung_that_fits(L):
    sizes = monotone(L, 11)
    for budget in budgets(sizes):
        fits = [r for r in range(L) if sizes[r] <= budget]
        if fits:
            assert R.search(lambda r: sizes[r], L, budget)[0] == fits[0]


def test_fits_at_rung_0_probes_once():
    for L in LENGTHS:
        rung, probes = R.search(lambda r: 100, L, 100)
        assert (rung, probes) == (0, [(0, 100)])


def test_unreachable_probes_the_two_ends_only():
    asked = []

    def size(r):
        asked.append(r)
        return 1000 - r
    with pytest.raises(ValueError):
        R.search(size, 50, 10)
    assert asked == [0, 49]


def test_a_single_rung():
    assert R.search(lambda r: 7, 1, 7) == (0, [(0, 7)])
    with pytest.raises(ValueError):
        R.search(lambda r: 8, 1, 7)
    from kompressor_amd import rate
    with pytest.raises(ValueError):
        rate.search(lambda r: 8, 1, 7)


def test_the_probe_bound_is_met_with_equality_somewhere():
    """2 + ceil(log2 L) is the bound of the rule, not a loose one: some budget needs that many."""
    for L in (2, 3, 9, 32, 33):
        sizes = list(range(10 * L, 0, -10))
        worst = max(len(R.search(lambda r: sizes[r], L, b)[1]) for b in range(10, 10 * L))
        assert worst <= R.max_probes(L) and worst >= R.max_probes(L) - 1
    assert R.max_probes(32) == 7 and R.max_probes(33) == 8 and R.max_probes(1) == 2 and math.ceil(math.log2(32768)) == 15


def test_budget():
    assert R.budget(1000, 4000, target_bits=4) == 500 and R.budget(1000, 4000, target_ratio=8) == 500
    assert R.budget(7, 28, target_bits=4.5) == 3 and R.budget(7, 28, target_ratio=3) == 9
    from kompressor_amd import rate
    for kw in ({'target_bits': 4}, {'target_ratio': 8}, {'target_bits': 0.37}, {'target_ratio': 1.7}):
        assert rate.budget_bytes(107520, 430080, **kw) == R.budget(107520, 430080, **kw)
