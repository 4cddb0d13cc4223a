"""Guard bands for the comparing call: kmp_code with KMP_CODER_COMPARE on arenas the test owns (guard_spec.py,
guard_capi.py) at the three pointer-shift modes.  Per launch: guards, shift bytes and both inputs
untouched; of ``out`` only the record and the partial records of the workgroups that ran are written,
nothing past KMP_COMPARE_BYTES; the record meets tests/metrics_spec.py (every word bit for bit but the
float32 ``sse``, which keeps the rule's bound) and the partials fold to it; two runs (0xA5 and 0x5A
surroundings) identical.  Counts lie around each 16-byte boundary of the three item sizes; unshifted
pointers at a multiple of the item run the vector kernel, every other case the element kernel."""

import math

import numpy as np
import pytest

import guard_capi as K
from guard_capi import T
import metrics_spec as M
import test_gpu_metrics as G

pytestmark = pytest.mark.gpu

COUNTS = (1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 4100, 4101)
WORDS = G.BYTES // 8


def bits(a):
    """An array as the unsigned array of its bit patterns (the arenas hold bytes; NaNs compare as bits)."""
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def judge_for(x, r, groups):
    """The predicate on ``out`` as uint64 words: True where a word misses the rule."""
    is_float = x.dtype == np.float32
    want = M.record(x, r)
    ww = M.words(want, is_float)
    exact = ('count', 'mismatch', 'max_abs', 'x_min', 'x_max') + (() if is_float else ('sse',))

    def wrong(words):
        bad = np.zeros(words.shape, bool)
        bad[:8] = words[:8] != ww
        if is_float:
            bad[3] = not M.sse_ok(M.from_words(words[:8], True)['sse'], x.size, want['sse'])
        part = {'count': 0, 'mismatch': 0, 'max_abs': 0.0, 'sse': 0.0 if is_float else 0, 'x_min': math.inf,
                'x_max': -math.inf}
        for g in range(groups):
            w = words[8 * (1 + g):8 * (2 + g)]
            bad[8 * (1 + g) + 6:8 * (2 + g)] = w[6:] != 0
            part = M.fold(part, M.from_words(w, is_float))
        ok = all(part[k] == want[k] for k in exact) and (not is_float or M.sse_ok(part['sse'], x.size, want['sse']))
        if not ok:
            bad[8:8 * (1 + groups)] = True
        return bad
    return wrong


@pytest.mark.parametrize('dtype', G.DTYPES, ids=G.IDS)
def test_compare(kom, dtype):
    code = G.CODE[np.dtype(dtype)]
    V, size = G.item(dtype), np.dtype(dtype).itemsize
    for n in COUNTS:
        x, r = G.pair(n, dtype, seed=13 * n)
        for shift in K.SHIFTS:
            # 'all' moves both inputs by one element; 'out' moves only the output, by its stated alignment
            vec = n % V == 0 and (shift != 'all' or size % 16 == 0)
            groups = min(G.GROUPS, -(-(n // V if vec else n) // G.THREADS))
            mask = np.zeros(WORDS, bool)
            mask[:8 * (1 + groups)] = True
            name = K.launch('kmp_code', [T('x', 'in', bits(x)), T('r', 'in', bits(r)),
                                         T('out', 'out', np.zeros(WORDS, np.uint64), mask=mask, align=8,
                                           judge=judge_for(x, r, groups))],
                            lambda fn, q: fn(0, G.COMPARE, code, q['r'], code, q['x'], n, q['out'], None), shift)
            assert name == 'compare'
