"""Guard bands for the SSIM call: kmp_code with KMP_CODER_SSIM on arenas the test owns (guard_spec.py,
guard_capi.py) at the three pointer-shift modes.  Per launch: guards, shift bytes and both inputs untouched; of
``out`` only the record and the partial records of the workgroups that ran are written -- the request the
caller put at ``out + 64`` reads back as it was, the slots of the workgroups that did not run and everything
past them still hold the sentinel; the record meets tests/ssim_spec.py and the partials fold to it; two runs
(0xA5 and 0x5A surroundings) identical.  Unshifted pointers and a width that is a multiple of 16 bytes take the
16-byte reads, every other case element reads."""

import math

import numpy as np
import pytest
import torch

import guard_capi as K
from guard_capi import T
import ssim_spec as S
import test_gpu_metrics as G
import test_gpu_ssim as U

pytestmark = pytest.mark.gpu

SHAPES = ((2, 1, 9, 16), (3, 1, 13, 19), (2, 8, 9, 32), (1, 39, 8, 10))


def judge_for(x, r, request, groups):
    """The predicate on ``out`` as uint64 words: True where a word misses the rule."""
    want = S.ssim(x, r)
    tol = S.TOL_F32 if x.dtype == np.float32 else S.TOL_INT

    def wrong(words):
        f = words.view(np.float64)
        bad = np.zeros(words.shape, bool)
        bad[0], bad[1] = words[0] != want['windows'], words[1] != want['skipped']
        bad[2] = not abs(f[2] / want['windows'] - want['ssim']) <= tol
        bad[3] = not abs(f[3] - want['min_ssim']) <= tol
        bad[4:8] = words[4:8] != 0
        bad[8:16] = words[8:16] != request.view(np.uint64)  # the request is only read
        part = words[16:16 + 8 * groups].reshape(groups, 8)
        pf = part.view(np.float64)
        ok = int(part[:, 0].sum()) == want['windows'] and int(part[:, 1].sum()) == want['skipped'] and \
            pf[:, 3].min() == f[3] and abs(math.fsum(pf[:, 2].tolist()) - f[2]) <= want['windows'] * 2.0 ** -50
        bad[16:16 + 8 * groups] = (part[:, 4:] != 0).any() or not ok
        return bad
    return wrong


@pytest.mark.parametrize('dtype', G.DTYPES, ids=G.IDS)
def test_ssim(kom, dtype):
    from kompressor_amd import _lib
    code = G.CODE[np.dtype(dtype)]
    words = _lib.SSIM_BYTES // 8
    for k, shape in enumerate(SHAPES):
        x, r = U.field(shape, dtype, seed=300 + k, levels=np.linspace(0.1, 0.9, shape[0]))
        request, _, _ = U.frame(x)
        groups = _lib.ssim_groups(x.size)
        assert groups < _lib.SSIM_GROUPS  # some workgroups do not run: their slots stay untouched
        mask = np.zeros(words, bool)
        mask[:16 + 8 * groups] = True

        def prepare(got):
            c = got['out']
            c.arena[K.G.GUARD + c.shift + 64:K.G.GUARD + c.shift + 128].copy_(
                torch.from_numpy(request.view(np.uint8).copy()))

        for shift in K.SHIFTS:
            name = K.launch('kmp_code', [T('x', 'in', G_bits(x)), T('r', 'in', G_bits(r)),
                                         T('out', 'out', np.zeros(words, np.uint64), mask=mask, align=8,
                                           judge=judge_for(x, r, request, groups))],
                            lambda fn, q: fn(0, _lib.CODER_SSIM, code, q['r'], code, q['x'], x.size, q['out'], None),
                            shift, prepare=prepare)
            assert name == 'ssim'


def G_bits(a):
    """An array as the unsigned array of its bit patterns (the arenas hold bytes)."""
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])
