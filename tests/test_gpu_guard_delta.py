"""Guard bands for the time-series kernels: kmp_code with KMP_CODER_DELTA on arenas the test owns
(guard_spec.py, guard_capi.py) at the three pointer-shift modes, both directions, all five dtypes.  Per
launch: guards, shift bytes and inputs untouched; nothing written outside the output; owned elements
bit-equal to tests/delta_spec.py; two runs (0xA5 and 0x5A surroundings) identical.  Unshifted pointers with
a count of whole 16-byte items run the 16-byte accesses, everything else the element form."""

import numpy as np
import pytest

import guard_capi as K
from guard_capi import T
import delta_spec as D

pytestmark = pytest.mark.gpu

DELTA = 13
CODE = {np.dtype(np.uint8): 0, np.dtype(np.int8): 5, np.dtype(np.uint16): 1, np.dtype(np.int16): 6,
        np.dtype(np.int32): 2}
# whole 16-byte items of every width (the 16-byte form when unshifted): one item of 8-bit samples, one
# workgroup of items, more than one workgroup; and counts that are not (the element form at any shift)
VEC_COUNTS = (16, 256 * 16, 2 * 256 * 16 + 16)
ELEMENT_COUNTS = (1, 15, 17, 4101, 2 * 256 * 16 + 5)


def arena_view(a):
    """The arenas know the unsigned dtypes and int32: the same bits (the launch is told the real dtype)."""
    a = np.ascontiguousarray(a)
    return a if a.dtype == np.int32 else a.view({1: np.uint8, 2: np.uint16}[a.dtype.itemsize])


def run(dtype, direction, n, shift):
    x, p = K.rand((n,), dtype, seed=n), K.rand((n,), dtype, seed=n + 7)
    want = D.sub(x, p) if direction == 0 else D.add(x, p)
    code = CODE[np.dtype(dtype)]
    name = K.launch('kmp_code', [T('pred', 'in', arena_view(p)), T('x', 'in', arena_view(x)),
                                 T('out', 'out', arena_view(want))],
                    lambda fn, q: fn(direction, DELTA, code, q['pred'], code, q['x'], n, q['out'], None), shift)
    assert name == 'delta'


@pytest.mark.parametrize('direction', (0, 1), ids=('encode', 'decode'))
@pytest.mark.parametrize('dtype', D.DTYPES, ids=[np.dtype(d).name for d in D.DTYPES])
def test_vector_form(kom, dtype, direction):
    for n in VEC_COUNTS:
        run(dtype, direction, n, 'none')


@pytest.mark.parametrize('direction', (0, 1), ids=('encode', 'decode'))
@pytest.mark.parametrize('dtype', D.DTYPES, ids=[np.dtype(d).name for d in D.DTYPES])
def test_element_form(kom, dtype, direction):
    for n in ELEMENT_COUNTS:
        for shift in K.SHIFTS:
            run(dtype, direction, n, shift)
    for n in VEC_COUNTS[:2]:  # whole items, but a pointer off the 16-byte grid
        for shift in ('all', 'out', {'pred': np.dtype(dtype).itemsize}, {'x': np.dtype(dtype).itemsize}):
            run(dtype, direction, n, shift)
