"""Guard bands for the kernels of masked float32 fields: kmp_code with KMP_CODER_FILL and KMP_CODER_RUNS on
arenas the test owns (guard_spec.py, guard_capi.py) at the three pointer-shift modes.  Per launch: guards,
shift bytes and inputs untouched; nothing written outside the output -- for RUNS nothing outside the runs'
extents --; owned elements bit-equal to tests/runs_spec.py; two runs (0xA5 and 0x5A surroundings)
identical.  Unshifted pointers run the 16-byte accesses, shifted ones the element form."""

import numpy as np
import pytest

import guard_capi as K
from guard_capi import T
import runs_spec as R

pytestmark = pytest.mark.gpu

KMP_I32, KMP_U32, KMP_I16 = 2, 4, 6
FILL, RUNS = 11, 12
FILL_BYTES, TILE = 16384, 2048
CODE = {np.dtype(np.int16): KMP_I16, np.dtype(np.int32): KMP_I32}
# around an item of 8 elements, a wave, a workgroup step, and three workgroups (2 * TILE + 1)
COUNTS = (1, 7, 8, 9, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 2 * TILE + 1)


def u(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def marked(n, dtype, seed):
    rng = np.random.default_rng(seed)
    info = np.iinfo(dtype)
    x = rng.integers(info.min + 1, int(info.max) + 1, size=n, dtype=np.int64).astype(dtype)
    at = 0
    while at < n:
        length = int(rng.integers(1, 120))
        if rng.random() < 0.4:
            x[at:at + length] = info.min
        at += length
    return x


@pytest.mark.parametrize('dtype', [np.int16, np.int32], ids=['int16', 'int32'])
def test_fill(kom, dtype):
    for n in COUNTS:
        x = marked(n, dtype, seed=n)
        if n == 2 * TILE + 1:
            x[TILE - 5:2 * TILE + 1] = np.iinfo(dtype).min  # the carry crosses a whole workgroup
        want = R.fill(x)
        for shift in K.SHIFTS:
            name = K.launch('kmp_code', [T('x', 'in', u(x)), T('out', 'out', u(want)),
                                         T('ws', 'scratch', np.zeros(FILL_BYTES, np.uint8), align=8)],
                            lambda fn, q: fn(0, FILL, 0, q['ws'], CODE[np.dtype(dtype)], q['x'], n, q['out'], None),
                            shift)
            assert name == 'fill'


def table_of(starts, lengths, bits):
    t = np.zeros((len(starts), 4), np.uint32)
    t[:, 0], t[:, 2], t[:, 3] = starts, lengths, bits
    return t


RUN_TABLES = [
    ([0], [1], [0x7fc00000]),
    ([1, 9, 80, 200, 300, 1000], [3, 63, 64, 65, 8, 9], [1, 2, 3, 4, 5, 6]),
    ([3, 11, 30000 - 17], [8, 12, 17], [0x7fc00000, 0x7f800000, 0x7fc00001]),  # adjacent; ending at numel
    ([7], [256 + 1], [0xff800000]),  # one element more than KMP_RUNS_PIECE
    ([7], [2048 + 1], [0xff800000]),
    ([9], [20001], [0xff800000]),
    (list(range(0, 2000, 2)), [1] * 1000, list(range(1000))),
]


@pytest.mark.parametrize('which', range(len(RUN_TABLES)))
def test_runs(kom, which):
    starts, lengths, bits = RUN_TABLES[which]
    table = table_of(starts, lengths, bits)
    numel = 30000
    want, owned = np.zeros(numel, np.uint32), np.zeros(numel, bool)
    for s, n, b in zip(starts, lengths, bits):
        want[s:s + n], owned[s:s + n] = b, True
    for shift in K.SHIFTS:
        name = K.launch('kmp_code', [T('table', 'in', table, align=16), T('out', 'out', want, mask=owned, align=4)],
                        lambda fn, q: fn(1, RUNS, 0, None, KMP_U32, q['table'], len(starts), q['out'], None), shift)
        assert name == 'runs'
