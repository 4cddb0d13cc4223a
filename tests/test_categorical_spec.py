"""The categorical path model against the oracle, and the census of paths its generators reach
(CPU only).  The GPU suite (``test_gpu_categorical_paths.py``) runs exactly these inputs: what is
asserted here is what it covers."""

import numpy as np
import pytest

import oracle.common
import categorical_spec as S

DTYPES = (np.uint8, np.uint16, np.int32, np.uint32)


@pytest.mark.parametrize('L', S.PATH_LS + (5, 65, 2000))
def test_model_matches_oracle(L):
    """The model's class and code equal the oracle's for every generated (row, rank), in every
    value dtype (ranks and classes past the dtype's range wrap, as the arrays handed to the
    kernels do)."""
    lg, rk, tags = S.elements(L)
    if L == 2000:
        lg, rk, tags = lg[::41], rk[::41], tags[::41]
    for dt in DTYPES:
        x = S.wrap(rk, dt)
        bits = 8 * np.dtype(dt).itemsize
        dec = oracle.common.decode_categorical(lg, x)
        enc = oracle.common.encode_categorical(lg, x)
        for i, (row, v) in enumerate(zip(lg, x)):
            bucket, cls = S.decode_path(row, int(v), L)
            assert np.asarray(cls).astype(dt) == dec[i], (L, dt.__name__, tags[i], int(v), bucket)
            bucket, code = S.encode_path(row, int(v), L, bits)
            assert code == int(enc[i]), (L, dt.__name__, tags[i], int(v), bucket)


def test_model_out_of_range_values():
    """No class matches a negative or far value (code 0); the decode clamps the rank."""
    for L in (8, 300):
        lg, _ = S.rows(L)
        lg = lg[::5]
        for dt, vals in ((np.int32, (-1, -L, -2**31, 2**31 - 1)), (np.uint32, (2**31, 2**32 - 1)),
                         (np.uint16, (65535,)), (np.uint8, (255,))):
            if dt == np.uint8 and L > 8:
                continue
            for v in vals:
                x = np.full(len(lg), v, dtype=dt)
                dec = oracle.common.decode_categorical(lg, x)
                enc = oracle.common.encode_categorical(lg, x)
                for i, row in enumerate(lg):
                    assert np.asarray(S.decode_path(row, v, L)[1]).astype(dt) == dec[i]
                    assert S.encode_path(row, v, L, 8 * np.dtype(dt).itemsize) == ('none', 0) and enc[i] == 0


@pytest.mark.parametrize('L', S.CENSUS_LS)
def test_decode_census(L):
    """Every required bucket of the vector decode -- per key path: each peel depth ending on one key
    and in a tie; all keys equal; for each class of differing-bit counts a first-round owner, a
    last-round owner and a last-round tie -- holds at least 4 generated elements, in every value
    dtype the GPU suite decodes at this L."""
    for dt in DTYPES:
        if dt == np.uint8 and L > 256:
            continue
        census = S.decode_census(L, dt)
        short = {b: census.get(b, 0) for b in S.REQUIRED_DECODE if census.get(b, 0) < 4}
        assert not short, (L, dt.__name__, short)
    print(f'\ndecode census L={L}: {S.format_census(S.decode_census(L, np.int32))}')


def test_generated_bit_spreads():
    """The spread rows differ in exactly the m low bits they were built for (P == m on both key
    paths, with and without the raw path's + 1; m > 24: at least m), so every class of P is there by
    construction."""
    for L in S.CENSUS_LS:
        lg, tags = S.rows(L)
        seen = set()
        for row, tag in zip(lg, tags):
            if ' spread m=' not in tag:
                continue
            m = int(tag.split('m=')[1].split()[0])
            kp, keys = S.decode_keys(row, L)
            assert kp == tag.split()[0]
            P = int(np.bitwise_or.reduce(keys ^ keys[0])).bit_length()
            # the bases have 24 low zero bits: wider offsets carry into the exponent, P >= m (4 digits)
            assert P == m if m <= 24 else m <= P <= 32, (L, tag, P)
            seen.add((kp, m))
        assert seen == {(kp, m) for kp, _ in S.BASES for m in S.SPREADS}


@pytest.mark.parametrize('L', S.PATH_LS)
def test_encode_census(L):
    """Every encode bucket holds at least 4 generated elements over the value dtypes ('alias': two
    classes match modulo 256, uint8 at L = 300 and 512 only)."""
    census = {}
    for dt in DTYPES:
        for b, c in S.encode_census(L, dt).items():
            if b == 'alias':
                assert dt == np.uint8 and L > 256
            census[b] = census.get(b, 0) + c
    want = [b for b in S.ENCODE_BUCKETS if b != 'alias' or L > 256]
    assert all(census.get(b, 0) >= 4 for b in want), (L, census)
    print(f'\nencode census L={L}: {S.format_census(census)}')


def test_alternating_order_changes_branch():
    """Consecutive elements of the range tests' input take different branches."""
    for L in (8, 252, 256):
        lg, rk = S.alternating(L)
        kinds = []
        for row, v in zip(lg, rk):
            b = S.decode_path(row, int(v), L)[0]
            kinds.append('ties' if b[-1] == 'ties' else 'peel' if b[1] == 'peel' else 'one' if b[3] == 1 else 'multi')
        assert kinds[:8] == ['peel', 'one', 'multi', 'ties'] * 2
        assert all(a != b for a, b in zip(kinds, kinds[1:]))


def test_range_plans():
    """The element counts of the range-length tests give every wave-range length the prefetch ring
    treats differently."""
    pers, lengths, lefts = set(), set(), set()
    ragged = empty_tail = False
    for n in S.range_sizes() + [8192]:
        per, lens = S.range_plan(n, 8)
        assert sum(lens) == n and max(lens) == per and len(lens) == 8192
        pers.add(per)
        lengths.update(lens)
        used = [x for x in lens if x]
        assert lens[:len(used)] == used  # empty ranges only trail
        ragged |= 0 < used[-1] < per
        empty_tail |= len(used) < len(lens) and 0 < used[-1] < per
        for x in used:
            if per >= 8 and x >= 8:
                rounds, left = S.ring_tail(x)
                assert rounds >= 1
                lefts.add(left)
    assert pers == set(range(1, 13))
    assert set(range(0, 13)) <= lengths  # no main loop and both tails (2..7), the main loop once (8), ...
    assert lefts == {4, 5, 6, 7}
    assert ragged and empty_tail
    assert S.range_plan(8193, 8)[1][4095:4098] == [2, 1, 0]
    # the existing long-range test: 139 per wave, 134 in the last
    per, lens = S.range_plan(8192 * 139 - 5, 8)
    assert per == 139 and lens[-1] == 134
    assert [S.ring_tail(x) for x in (1, 7, 8, 9, 11, 12, 139)] == [(0, 1), (0, 7), (1, 4), (1, 5), (1, 7), (2, 4),
                                                                  (33, 7)]
    # the sampled sizes at L = 256 / 252 stay on the 2 048-block grid
    for L in (252, 256):
        for per in (2, 7, 8, 9):
            assert S.range_plan(8192 * per - 5, L)[0] == per
