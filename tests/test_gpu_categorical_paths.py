"""The categorical coder on inputs that reach every decode, encode and range path.

The rows come from ``categorical_spec``'s generators, whose census of control paths the CPU suite
asserts (``test_categorical_spec.py``).  Every comparison is bit for bit against the oracle's
stable argsort, and every GPU call is made twice with equal results (stale histogram bins or owner
slots would differ between runs or between neighbours).  Aligned logits take the vector kernels
(L % 4 == 0, L <= 512); logits that start 4 bytes past a 16-byte boundary take the scalar ones.
"""

import numpy as np
import pytest
import torch

import oracle.common
import categorical_spec as S

pytestmark = pytest.mark.gpu

ALIGN = ('aligned', 'shifted')


def place(logits, align):
    """The logits on the GPU: 16-byte aligned, or starting 4 bytes past a 16-byte boundary."""
    src = logits if torch.is_tensor(logits) else torch.from_numpy(np.array(logits, dtype=np.float32))
    if align == 'aligned':
        lg = src.cuda().contiguous()
        assert lg.data_ptr() % 16 == 0
        return lg
    buf = torch.empty(src.numel() + 4, dtype=torch.float32, device='cuda')
    lg = buf[1:1 + src.numel()].view(src.shape)
    lg.copy_(src)
    assert lg.data_ptr() % 16 == 4
    return lg


def twice(fn, lg, xg):
    a = fn(lg, xg).cpu().numpy()
    b = fn(lg, xg).cpu().numpy()
    assert np.array_equal(a, b), f'{fn.__name__}: two runs on the same input differ'
    return a


def check(kom, direction, lg, logits, x, L, idx=None):
    """One direction on the GPU (twice) against the oracle, at ``idx`` (default: everywhere); a
    mismatch names the model's bucket of the first wrong element."""
    fn = kom.utils.decode_categorical if direction == 'decode' else kom.utils.encode_categorical
    got = twice(fn, lg, torch.from_numpy(x).cuda())
    assert got.dtype == x.dtype and got.shape == x.shape
    if idx is not None:
        got, x = got[idx], x[idx]
    ref = oracle.common.decode_categorical if direction == 'decode' else oracle.common.encode_categorical
    want = ref(logits, x)
    bad = np.flatnonzero(got != want)
    if len(bad):
        i = int(bad[0])
        e = i if idx is None else int(idx[i])
        v = int(x[i])
        bucket = (S.decode_path(logits[i], v, L)[0] if direction == 'decode'
                  else S.encode_path(logits[i], v, L, 8 * x.dtype.itemsize)[0])
        raise AssertionError(f'{direction} L={L} {x.dtype}: {len(bad)} of {len(want)} wrong; first at element {e}: '
                             f'value {v}, got {int(got[i])}, want {int(want[i])}, model bucket {bucket}')
    return got


def value_dtypes(L):
    return (np.uint8, np.uint16, np.int32, np.uint32) if L <= 256 else (np.uint16, np.int32, np.uint32)


@pytest.mark.parametrize('align', ALIGN)
@pytest.mark.parametrize('L', S.PATH_LS)
def test_decode_paths(kom, L, align):
    """Every generated row at every rank of ``ranks_for(L)``: both key paths, every peel depth, every
    digit width and round count of the radix select, owner slots and tie walks (vector kernels, FULL
    and not, one and two slots; shifted: ``categorical_decode_select_kernel`` E = 1, 4, 8)."""
    logits, ranks, _ = S.elements(L)
    lg = place(logits, align)
    for dt in value_dtypes(L):
        check(kom, 'decode', lg, logits, S.wrap(ranks, dt), L)
    if align == 'aligned':
        print(f'\ndecode census L={L}: {S.format_census(S.decode_census(L, np.int32))}')


@pytest.mark.parametrize('align', ALIGN)
def test_decode_paths_select_e2(kom, align):
    """L = 128: the two-slot instance of the scalar select (shifted) beside the vector kernel."""
    logits, ranks, _ = S.elements(128)
    lg = place(logits, align)
    for dt in value_dtypes(128):
        check(kom, 'decode', lg, logits, S.wrap(ranks, dt), 128)


def test_decode_paths_unstaged(kom):
    """L = 2000: ``categorical_kernel``'s decode with the logits read from global memory."""
    L = 2000
    logits, ranks, _ = S.elements(L)
    n = len(S.ranks_for(L))
    rows = np.linspace(0, len(logits) // n - 1, 32).astype(np.int64)
    idx = (rows[:, None] * n + np.arange(n)).ravel()
    logits, ranks = logits[idx], ranks[idx]
    lg = place(logits, 'aligned')
    for dt in (np.uint16, np.int32):
        check(kom, 'decode', lg, logits, S.wrap(ranks, dt), L)
        check(kom, 'encode', lg, logits, S.wrap(ranks, dt), L)


@pytest.mark.parametrize('align', ALIGN)
@pytest.mark.parametrize('L', S.PATH_LS)
def test_encode_paths(kom, L, align):
    """The same rows with classes that have a unique logit (packed-count fast path), a tied logit, a
    NaN logit, no match at all, and -- uint8 at L = 300 and 512 -- two matching classes g and g + 256,
    of which the smaller rank wins."""
    logits, values, _ = S.elements(L)
    lg = place(logits, align)
    for dt in (np.uint8, np.uint16, np.int32, np.uint32):
        check(kom, 'encode', lg, logits, S.wrap(values, dt), L)
    if align == 'aligned':
        census = {}
        for dt in (np.uint8, np.uint16, np.int32, np.uint32):
            for b, c in S.encode_census(L, dt).items():
                census[b] = census.get(b, 0) + c
        print(f'\nencode census L={L}: {S.format_census(census)}')


@pytest.mark.parametrize('align', ALIGN)
@pytest.mark.parametrize('dt,L,values', [
    (np.int32, 8, (-1, -8, -2**31, 2**31 - 1)),
    (np.int32, 256, (-1, -256, -2**31, 2**31 - 1)),
    (np.int32, 300, (-1, -300, -2**31, 2**31 - 1)),
    (np.int32, 5, (-1, -5, -2**31, 2**31 - 1)),
    (np.uint32, 8, (2**31, 2**32 - 1)),
    (np.uint32, 300, (2**31, 2**32 - 1)),
    (np.uint16, 8, (65535,)),
    (np.uint16, 300, (65535,)),
    (np.uint8, 8, (255,)),
])
def test_out_of_range_values(kom, dt, L, values, align):
    """Values no class matches encode to 0 and ranks outside [0, L) clamp, as the oracle has it:
    negatives down to INT32_MIN, INT32_MAX, uint32 values at and above 2^31, the largest uint16 and
    uint8.  Mixed with in-range values so that neighbours in a wave's range take other branches."""
    logits, _ = S.rows(L)
    pattern = list(values) + [0, L - 1, values[0], L // 2]
    x = S.wrap(np.resize(np.asarray(pattern, dtype=np.int64), len(logits)), dt)
    lg = place(logits, align)
    enc = check(kom, 'encode', lg, logits, x, L)
    dec = check(kom, 'decode', lg, logits, x, L)
    out = np.isin(x, S.wrap(values, dt))
    assert not enc[out].any()
    xi = x.astype(np.int64)
    first = oracle.common.decode_categorical(logits, np.zeros(len(x), dt))
    last = oracle.common.decode_categorical(logits, np.full(len(x), L - 1, dt))
    assert out.sum() >= len(x) // 3 and np.all((xi[out] < 0) | (xi[out] >= L))
    assert np.array_equal(dec[out], np.where(xi < 0, first, last)[out])


def cycled(base_logits, base_values, n, dt):
    """n elements taken cyclically from the base rows: the logits gathered on the GPU, the index and
    the values on the host."""
    idx = np.arange(n) % len(base_logits)
    lg = torch.from_numpy(np.array(base_logits, dtype=np.float32)).cuda()[torch.from_numpy(idx).cuda()]
    return idx, lg, S.wrap(base_values[idx], dt)


@pytest.mark.parametrize('dt', [np.uint8, np.int32])
@pytest.mark.parametrize('per', list(range(2, 13)) + [0])
def test_range_lengths(kom, per, dt):
    """L = 8, every element against the oracle: n = 8192 per - r gives every wave a range of `per`
    elements (no main loop of the prefetch ring and both tails for per < 8, the main loop once or
    twice and 4 to 7 elements left for per 8..12), the last range ragged (r = 1, 5) or followed by
    waves with nothing to do; per = 0 stands for n = 8193 (4 096 ranges of 2, one of 1, the rest
    empty).  Consecutive elements alternate peel, one-round, multi-round and tie rows."""
    L = 8
    base, ranks = S.alternating(L)
    rng = np.random.default_rng(per)
    for n in ([8193] if per == 0 else [8192 * per - r for r in (0, 1, 5)]):
        assert S.range_plan(n, L)[0] == (2 if per == 0 else per)
        idx, lg, r = cycled(base, ranks, n, dt)
        assert lg.data_ptr() % 16 == 0
        logits = base[idx]
        check(kom, 'decode', lg, logits, r, L)
        check(kom, 'encode', lg, logits, S.wrap(rng.integers(0, L + 1, n), dt), L)


@pytest.mark.parametrize('per', [2, 7, 8, 9])
@pytest.mark.parametrize('L', [256, 252])
def test_range_lengths_wide(kom, L, per):
    """L = 256 (every class exists) and 252: all elements through decode(encode(x)) == x, and the
    first and last element of every wave's range plus 2 000 sampled ones against the oracle."""
    base, ranks = S.alternating(L)
    rng = np.random.default_rng(per)
    for r_ in (0, 1, 5):
        n = 8192 * per - r_
        assert S.range_plan(n, L)[0] == per
        idx, lg, r = cycled(base, ranks, n, np.uint8)
        assert lg.data_ptr() % 16 == 0
        x = rng.integers(0, L, n).astype(np.uint8)
        firsts = np.arange(0, n, per)
        sample = np.unique(np.concatenate([firsts, np.minimum(firsts + per - 1, n - 1), rng.integers(0, n, 2000)]))
        logits = base[idx[sample]]
        enc = twice(kom.utils.encode_categorical, lg, torch.from_numpy(x).cuda())
        dec = twice(kom.utils.decode_categorical, lg, torch.from_numpy(enc).cuda())
        assert np.array_equal(dec, x)  # every x < L <= 256: decode inverts encode
        assert np.array_equal(enc[sample], oracle.common.encode_categorical(logits, x[sample]))
        check(kom, 'decode', lg, logits, r, L, idx=sample)


@pytest.mark.parametrize('L,dt,align', [(5, np.int32, 'aligned'), (65, np.uint16, 'aligned'), (8, np.uint8, 'shifted')])
def test_scalar_grid_stride(kom, L, dt, align):
    """More elements than the scalar kernels' 65 536 blocks of 4 waves hold: every wave loops, and
    ``categorical_kernel`` refills its LDS stage with the next element's logits (L = 5: the encode
    and the one-slot select; L = 65: the two-slot select; L = 8 off alignment).  L = 5 and 8: every
    element against the oracle; L = 65: the first and last 2 000 and 2 000 sampled ones."""
    n = 262144 + 517
    base, ranks, _ = S.elements(L)
    idx, lg, r = cycled(base, ranks, n, dt)
    lg = place(lg, align)
    rng = np.random.default_rng(L)
    x = S.wrap(rng.integers(0, L + 1, n), dt)
    sample = None
    if L == 65:
        sample = np.unique(np.concatenate([np.arange(2000), np.arange(n - 2000, n), rng.integers(0, n, 2000)]))
    logits = base[idx] if sample is None else base[idx[sample]]
    check(kom, 'decode', lg, logits, r, L, idx=sample)
    check(kom, 'encode', lg, logits, x, L, idx=sample)
