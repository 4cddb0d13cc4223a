"""The conditions test_gpu_linear_casts.py relies on, checked on the CPU from the oracle alone: the
class cycle reaches every channel, the saturating channels are decided everywhere, the crossing
channels do cross, the expected cells of the two arithmetics agree where both make a claim, the
predictions a coder used can be read back from its maps, and the oracle itself is lossless on these
predictors for uint8, uint16, int32 and uint32 samples."""

import numpy as np
import pytest

from oracle import predictors as OP
from oracle.common import cast_from_f32

import linear_cast_spec as S

U8, U16, I32, U32 = np.uint8, np.uint16, np.int32, np.uint32

CASES = [(3, 0, (2, 9, 10, 12, 1), U16), (3, 1, (2, 8, 9, 7, 1), U8), (3, 0, (1, 5, 6, 7, 3), U8),
         (2, 0, (3, 33, 20, 1), U8), (2, 1, (2, 30, 31, 2), U16), (2, 2, (2, 17, 17, 1), U16)]
CASES_32 = [(3, 0, (2, 9, 10, 12, 1), I32), (3, 1, (2, 9, 10, 12, 1), U32), (3, 0, (1, 8, 9, 7, 2), U32),
            (2, 0, (2, 17, 20, 1), I32), (2, 1, (2, 17, 20, 1), U32), (2, 2, (2, 17, 20, 1), I32)]


@pytest.mark.parametrize('dtype', [U8, U16])
@pytest.mark.parametrize('ndim', [2, 3])
def test_every_class_meets_every_channel(ndim, dtype):
    cyc = S.classes(dtype, ndim)
    sets = S.weight_sets(dtype, 0, ndim)
    K = S.NPRED[ndim]
    names = {c[:2] for c in cyc}
    assert len(names) == len(cyc) == len(sets)
    if ndim == 3:
        assert len([c for c in cyc if c[0] == 'const']) == 19
    assert {('sat', -1.2), ('sat', 1.2)} <= names and any(c[0] == 'cross' for c in cyc)
    for k in range(K):
        assert {ws.cls[k][:2] for ws in sets} == names, f'channel {k}'
    for ws in sets:
        for k, c in enumerate(ws.cls):
            if c[0] == 'const':  # non-finite (and every other constant) bias: a zero column
                assert not ws.w[:, k].any() and (ws.b[k] == c[2] or np.isnan(c[2]))
            else:
                assert np.isfinite(ws.b[k]) and ws.w[:, k].all()
        assert np.isfinite(ws.w).all()


def test_constants_cast_as_named():
    """The spec's constants against the cast written out by hand, for both sample sizes."""
    for dtype in (U8, U16):
        M = np.iinfo(dtype).max
        want = {'-0': 0, 'denormal': 0, '0.999': 0, '-1e-3': 0, '-0.5': 0, '-1': 0, '-1.2M': 0, 'M-0.5': M - 1, 'M': M,
                'M+0.5': M, 'M+1': M, '1.2M': M, '2^31': M, '2^32-256': M, '2^32': M, '3e38': M, '+inf': M, '-inf': 0,
                'nan': 0}
        got = {n: int(cast_from_f32(c, dtype)) for _, n, c in S.constant_classes(dtype)}
        assert got == want


@pytest.mark.parametrize('ndim,p,shape,dtype', CASES)
def test_expected_cells_conditions(ndim, p, shape, dtype):
    M = int(np.iinfo(dtype).max)
    hi = S.data(shape, dtype)
    padded, dims, window, feats = S.window_and_features(hi, p, ndim)
    gt = S.gt_maps(padded, ndim, dims)
    enc, dec = S.coders(S.ons(ndim), dtype)
    crossed = {'below': False, 'above': False, 'inside': False}
    for ws in S.weight_sets(dtype, p, ndim):
        v32 = S.chain(feats, ws)
        cells32, all_decided = S.expected_cells(feats, ws, dtype, 'f32')
        cells, decided = S.expected_cells(feats, ws, dtype, 'bf16x2')
        assert all_decided.all() and cells32.dtype == cells.dtype == np.dtype(dtype)
        ix = lambda k: (slice(None),) * (ndim + 1) + (k,)  # noqa: E731
        for k in ws.channels('const'):
            c = ws.cls[k][2]
            # the chain leaves a constant channel at its bias (-0 + 0 * f = +0 is the one change of bits)
            want_bits = np.float32(0.0 if c == 0 else c).view(np.uint32)
            assert (v32[ix(k)].view(np.uint32) == want_bits).all(), ws.cls[k]
        for k in ws.channels('sat'):  # a condition, not a measurement: nothing is excluded
            assert decided[ix(k)].all(), f'rotation {ws.rotation} channel {k}: undecided saturating cells'
            assert (cells[ix(k)] == (0 if ws.cls[k][1] < 0 else M)).all()
        # where both arithmetics make a claim they make the same one
        assert np.array_equal(cells[decided], cells32[decided])
        assert decided.sum() == decided[ix(0)].size * (len(ws.channels('const')) + len(ws.channels('sat')))
        vc = np.stack([v32[ix(k)] for k in ws.channels('cross')]) if ws.channels('cross') else np.zeros(0)
        crossed['below'] |= bool((vc <= -1).any())
        crossed['above'] |= bool((vc >= M + 1).any())
        crossed['inside'] |= bool(((vc > 0) & (vc < M)).any())
        if ws.channels('cross'):
            assert (vc <= -1).any() or (vc >= M + 1).any()
            assert ((vc > 0) & (vc < M)).any()
        # the mask through the aggregation; the predictions read back from the oracle's own maps
        fn = OP.linear_predictions_fn(p, ws.w, ws.b, ndim)
        with np.errstate(invalid='ignore'):
            lo, (maps, edims) = S.ons(ndim).encode(fn, enc, hi, padding=p)
            assert np.array_equal(S.ons(ndim).decode(fn, dec, lo, (maps, edims), padding=p), hi)
        assert tuple(edims) == tuple(dims)
        want_maps, dmaps = S.expected_maps(cells, decided, ndim, dims)
        got = S.recover_predictions(gt, maps)
        pm32, full = S.expected_maps(cells32, all_decided, ndim, dims)
        for g, w32, f in zip(got, pm32, full):
            assert f.all() and np.array_equal(g, w32)
        assert not S.mismatches(got, want_maps, dmaps, ws)
        cmap = 3 if ndim == 3 else 2  # the C map is one channel: decided iff that channel is
        assert dmaps[cmap].all() == (ws.cls[6 if ndim == 3 else 4][0] != 'cross')
    assert all(crossed.values()), crossed


def test_mismatch_report_names_the_classes():
    hi = S.data((2, 8, 9, 7, 1), U8)
    padded, dims, window, feats = S.window_and_features(hi, 0, 3)
    ws = S.weight_sets(U8, 0, 3)[3]
    cells, decided = S.expected_cells(feats, ws, U8, 'bf16x2')
    want, dmaps = S.expected_maps(cells, decided, 3, dims)
    k = ws.channels('const')[0]
    wrong = cells.copy()
    wrong[:, :, :, :, k] ^= 1
    got, _ = S.expected_maps(wrong, decided, 3, dims)
    lines = S.mismatches(got, want, dmaps, ws)
    assert lines and all('channel classes' in ln and 'rotation 3' in ln for ln in lines)


@pytest.mark.parametrize('ndim,p,shape,dtype', CASES_32)
def test_wide_samples_oracle(ndim, p, shape, dtype):
    info = np.iinfo(dtype)
    hi = S.data(shape, dtype)
    for v in (info.min, info.max, 0, 2 ** 24 + 1):
        assert (hi == v).any()
    padded, dims, window, feats = S.window_and_features(hi, p, ndim)
    enc, dec = S.coders(S.ons(ndim), dtype)
    sets = S.weight_sets_32(dtype, p, ndim)
    seen, ends = set(), {'low': 0.0, 'high': 0.0}
    for ws in sets:
        cells, _ = S.expected_cells(feats, ws, dtype, 'f32')
        for k in ws.channels('const'):
            seen.add(ws.cls[k][1])
            assert (cells[(slice(None),) * (ndim + 1) + (k,)] == cast_from_f32(ws.cls[k][2], dtype)).all()
        if ws.rotation == 0:  # the spread biases saturate a good part of the cells at each end
            ends['low'] = max(ends['low'], (cells == info.min).mean())
            ends['high'] = max(ends['high'], (cells == info.max).mean())
            assert (cells == info.min).mean() < 0.6 and (cells == info.max).mean() < 0.6
        fn = OP.linear_predictions_fn(p, ws.w, ws.b, ndim)
        with np.errstate(invalid='ignore'):
            lo, (maps, edims) = S.ons(ndim).encode(fn, enc, hi, padding=p)
            assert np.array_equal(S.ons(ndim).decode(fn, dec, lo, (maps, edims), padding=p), hi)
    assert seen == set(S.WIDE_CONSTANTS)
    assert ends['low'] > 0.05 and ends['high'] > 0.05, ends


def test_split_chunk_splits():
    from oracle.common import yield_chunks
    for shape, ndim in (((2, 8, 9, 7, 1), 3), ((1, 6, 32, 32, 1), 3), ((2, 17, 20, 1), 2), ((2, 12, 64, 64, 1), 3)):
        chunk = S.split_chunk(shape, ndim)
        L = [(s + (s + 1) % 2 + 1) // 2 for s in shape[1:1 + ndim]]
        counts = [len(list(yield_chunks(ext, c))) for ext, c in zip(L, chunk)]
        assert sorted(counts)[-1] >= 2 and sorted(counts)[:-1] == [1] * (ndim - 1), (shape, chunk, counts)
    assert S.split_chunk((1, 5, 6, 7, 3), 3) == (4, 4, 4)  # 3 x 4 x 4 nodes: nothing to split
