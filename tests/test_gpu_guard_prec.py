"""Guard bands for the relative-error float32 quantisers: kmp_code with KMP_CODER_PREC codes on arenas the
test owns (guard_spec.py, guard_capi.py) at the three pointer-shift modes.  Per launch: guards, shift
bytes and inputs untouched; nothing written outside the output; owned elements bit-equal to
tests/prec_spec.py; two runs (0xA5 and 0x5A surroundings) identical.  Counts lie around each 16-byte
boundary of both sides of a launch; a count that is a multiple of four at unshifted pointers runs the
vector kernel, every other case the element kernel, in both directions."""

import numpy as np
import pytest

import guard_capi as K
from guard_capi import T
import prec_spec as P

pytestmark = pytest.mark.gpu

KMP_F32, KMP_I32, KMP_I16 = 3, 2, 6
CODE = {np.dtype(np.int16): (8, KMP_I16), np.dtype(np.int32): (9, KMP_I32)}
# float32 / int32: 4 per 16 bytes; int16: 8 per 16 bytes; 4096 + 4: more than one block of vector items
COUNTS = (1, 3, 4, 5, 7, 8, 9, 12, 15, 16, 17, 4100, 4101)


def coder_arg(dtype, m):
    return CODE[np.dtype(dtype)][0] | ((m + 1) << 8)


def u(a):
    """An array as the unsigned array of its bit patterns (the arenas hold bytes; NaNs compare as bits)."""
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def samples(n, m, dtype, seed):
    """Random bit patterns, values of a few units, and the rule's edges."""
    x = P.random_bits(n, seed)
    x[::2] = np.random.default_rng(seed + 1).uniform(-4, 4, size=n).astype(np.float32)[::2]
    ka = P.known_answers(m, dtype)[0]
    k = min(n, ka.size)
    x[n - k:] = ka[:k]
    return x


@pytest.mark.parametrize('m', [0, 7, 8, 22])
@pytest.mark.parametrize('dtype', [np.int16, np.int32], ids=['int16', 'int32'])
def test_code(kom, dtype, m):
    code, ncode = CODE[np.dtype(dtype)]
    coder = coder_arg(dtype, m)
    for n in COUNTS:
        x = samples(n, m, dtype, seed=n)
        enc = P.encode_bits(x, m, dtype)
        ints = np.random.default_rng(n).integers(np.iinfo(dtype).min, int(np.iinfo(dtype).max) + 1, size=n,
                                                 dtype=np.int64).astype(dtype)
        ints[:min(n, 4)] = np.array([np.iinfo(dtype).min, 0, -1, np.iinfo(dtype).max], dtype)[:min(n, 4)]
        dec = P.dequant(ints, m)
        for shift in K.SHIFTS:
            name = K.launch('kmp_code', [T('x', 'in', u(x)), T('out', 'out', u(enc))],
                            lambda fn, q: fn(0, coder, 0, None, KMP_F32, q['x'], n, q['out'], None), shift)
            assert name == 'code'
            name = K.launch('kmp_code', [T('x', 'in', u(ints)), T('out', 'out', u(dec))],
                            lambda fn, q: fn(1, coder, 0, None, ncode, q['x'], n, q['out'], None), shift)
            assert name == 'code'
