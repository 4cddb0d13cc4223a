"""The LinearPredictor's cast (truncate, saturate, NaN -> 0) on every kernel that writes it, at the
values where the hand-written forms could disagree: predictions below zero, at and past the sample
maximum, at and past 2^32, infinite and NaN (tests/linear_cast_spec.py builds the predictors and
the expected cells; test_linear_cast_spec.py checks its conditions on the CPU).

Per family and sample type, for every rotation of the class cycle over the channels:
  * arith='f32': lowres, maps, float32 cell values (as bits) and cells equal the oracle;
  * arith='bf16x2' / 'auto': the predictions read back from the fused kernel's maps, and the cells of
    predict_cells, equal the specification wherever it decides (every constant and saturating
    channel, on every row of every plane); fused, generic and callable paths give the same bits;
  * a volume or image coded by one path decodes losslessly by the others: the same kernel, the
    generic path (KMP_DISABLE_LINEAR_FUSED), chunked, and through the callback path.
32-bit samples (int32 with the raw coder, uint32) run the f32 predictor on the generic path."""

import numpy as np
import pytest
import torch

from oracle import predictors as OP
from oracle.common import cast_from_f32

import linear_cast_spec as S

pytestmark = pytest.mark.gpu

U8, U16, I32, U32 = np.uint8, np.uint16, np.int32, np.uint32
TORCH = {U8: torch.uint8, U16: torch.uint16, I32: torch.int32, U32: torch.uint32}


def _last(kom):
    return kom._lib.lib.kmp_last_launch().decode()


def _launch(family, direction):
    return f'{direction}_generic' if family == 'generic' else f'{family}_{direction}'


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b)) and len(a) == len(b)


def _decode_routes(kom, ns, pred, dec, lo, maps, dims, p, hi, family, chunk, what):
    """A fresh encoding decoded by its own path, the generic path, chunked and through the callback."""
    enc_ = (maps, dims)
    assert np.array_equal(ns.decode(pred, dec, lo, enc_, padding=p), hi), f'{what}: own path'
    assert _last(kom) == _launch(family, 'decode'), what
    with kom._lib.option('KMP_DISABLE_LINEAR_FUSED', 1):
        assert np.array_equal(ns.decode(pred, dec, lo, enc_, padding=p), hi), f'{what}: generic decode'
        assert _last(kom) == 'decode_generic', what
    assert np.array_equal(ns.decode_chunks(pred, dec, lo, enc_, chunk=chunk, padding=p), hi), f'{what}: chunked'
    assert np.array_equal(ns.decode(lambda x: pred(x), dec, lo, enc_, padding=p), hi), f'{what}: callback'


# ---------------------------------------------------------------------------------------------
# arith='f32': everything equals the oracle
# ---------------------------------------------------------------------------------------------

F32 = [
    # (family, ndim, p, shape, dtype, KMP_LINEAR_F32_MFMA)
    ('linear3y', 3, 0, (1, 6, 32, 32, 1), U16, 0), ('linear3y', 3, 0, (2, 8, 32, 64, 1), U8, 0),
    ('linear3y', 3, 0, (1, 7, 32, 32, 1), U16, 0),
    ('linear3d', 3, 0, (2, 17, 30, 16, 1), U16, 0), ('linear3d', 3, 0, (2, 9, 15, 32, 1), U16, 0),
    ('linear3d', 3, 0, (1, 9, 14, 128, 1), U8, 0),
    ('linear3dp', 3, 1, (2, 9, 14, 32, 1), U16, 0), ('linear3dp', 3, 1, (2, 9, 14, 32, 1), U8, 0),
    ('wave2d', 2, 0, (3, 64, 64, 1), U16, 0), ('wave2d', 2, 0, (2, 37, 128, 1), U8, 0),
    # the generic row kernel computing the image cells itself (fuse_lin2d)
    ('generic', 2, 0, (2, 31, 45, 1), U8, 0), ('generic', 2, 0, (2, 31, 45, 1), U16, 0),
    ('generic', 2, 1, (2, 31, 45, 1), U8, 0), ('generic', 2, 1, (2, 31, 45, 1), U16, 0),
    # the generic two-pass path on both f32 cell kernels, and the per-element kernel (3 channels)
    ('generic', 3, 1, (2, 8, 9, 7, 1), U16, 0), ('generic', 3, 1, (2, 8, 9, 7, 1), U16, 1),
    ('generic', 2, 2, (2, 17, 17, 1), U8, 0), ('generic', 2, 2, (2, 17, 17, 1), U8, 1),
    ('generic', 3, 0, (1, 5, 6, 7, 3), U8, 0),
]


def _id(c):
    return f'{c[0]}-p{c[2]}-{"x".join(map(str, c[3]))}-{np.dtype(c[4]).name}' + ('-mfma' if len(c) > 5 and c[5] else '')


@pytest.mark.parametrize('family,ndim,p,shape,dtype,mfma', F32, ids=[_id(c) for c in F32])
def test_f32_casts(kom, family, ndim, p, shape, dtype, mfma):
    ns, ons = (kom.volume, S.ons(3)) if ndim == 3 else (kom.image, S.ons(2))
    (enc, dec), (oenc, _) = S.coders(ns, dtype), S.coders(ons, dtype)
    hi = S.data(shape, dtype)
    _, _, window, feats = S.window_and_features(hi, p, ndim)
    chunk = S.split_chunk(shape, ndim)
    with kom._lib.option('KMP_LINEAR_F32_MFMA', mfma):
        for ws in S.weight_sets(dtype, p, ndim):
            what = f'rotation {ws.rotation}'
            pred = kom.LinearPredictor(ws.w, ws.b, p, ndim, arith='f32')
            with np.errstate(invalid='ignore'):
                want_lo, (want_maps, want_dims) = ons.encode(OP.linear_predictions_fn(p, ws.w, ws.b, ndim), oenc, hi,
                                                             padding=p)
            lo, (maps, dims) = ns.encode(pred, enc, hi, padding=p)
            assert _last(kom) == _launch(family, 'encode'), what
            assert tuple(dims) == tuple(want_dims) and np.array_equal(lo, want_lo), what
            gt = S.gt_maps(S.ons(ndim).pad_highres(hi)[0], ndim, dims)
            lines = S.mismatches(S.recover_predictions(gt, maps), S.recover_predictions(gt, want_maps),
                                 [np.ones(m.shape, bool) for m in want_maps], ws)
            assert not lines and _same(maps, want_maps), '\n'.join(lines)
            # the cell kernel: float32 values as bits (NaN and -0 count), then the cast
            cells, cells_f = pred.predict_cells(window, with_f32=True)
            assert _last(kom) == ('linear_mfma' if mfma else 'linear_valu')
            exact = S.chain(feats, ws)
            assert np.array_equal(cells_f.view(np.uint32), exact.view(np.uint32)), what
            assert np.array_equal(cells, cast_from_f32(exact, dtype)), what
            # the other encoders give the same bytes, so any of them stands for all in the decodes
            with kom._lib.option('KMP_DISABLE_LINEAR_FUSED', 1):
                lo_g, (maps_g, _) = ns.encode(pred, enc, hi, padding=p)
                assert _last(kom) == 'encode_generic'
            lo_c, (maps_c, _) = ns.encode(lambda x: pred(x), enc, hi, padding=p)
            assert np.array_equal(lo_g, lo) and _same(maps_g, maps), f'{what}: generic encode'
            assert np.array_equal(ns.decode(pred, dec, lo_g, (maps_g, dims), padding=p), hi), f'{what}: generic -> own'
            assert np.array_equal(lo_c, lo) and _same(maps_c, maps), f'{what}: callback encode'
            _decode_routes(kom, ns, pred, dec, lo, maps, dims, p, hi, family, chunk, what)


# ---------------------------------------------------------------------------------------------
# arith='bf16x2' and 'auto'
# ---------------------------------------------------------------------------------------------

BF = [
    ('linear3m', 3, 0, (2, 16, 32, 32, 1), U16), ('linear3m', 3, 0, (2, 8, 32, 64, 1), U8),
    ('linear3m', 3, 0, (2, 15, 32, 32, 1), U16),
    # both row widths, both plane heights, an odd depth (the last plane has no C cells), a small workspace
    *[('linear3pm', 3, 1, shape, dt) for dt in (U8, U16)
      for shape in ((1, 8, 32, 64, 1), (1, 7, 64, 32, 1), (1, 6, 32, 32, 1), (2, 12, 64, 64, 1))],
    # the generic matrix-core cell kernel
    ('generic', 3, 0, (2, 9, 10, 12, 1), U16), ('generic', 3, 1, (2, 8, 9, 7, 1), U16),
    ('generic', 2, 0, (3, 33, 20, 1), U8), ('generic', 2, 1, (2, 30, 31, 2), U16),
]


@pytest.mark.parametrize('family,ndim,p,shape,dtype', BF, ids=[_id(c) for c in BF])
def test_bf16x2_casts(kom, family, ndim, p, shape, dtype):
    ns, ons = (kom.volume, S.ons(3)) if ndim == 3 else (kom.image, S.ons(2))
    (enc, dec), (oenc, _) = S.coders(ns, dtype), S.coders(ons, dtype)
    hi = S.data(shape, dtype)
    padded, dims0, window, feats = S.window_and_features(hi, p, ndim)
    gt_full = ons.maps_from_highres(padded)
    gt = S.gt_maps(padded, ndim, dims0)
    chunk = S.split_chunk(shape, ndim)
    auto_ok = ndim == 3 and p == 1
    for ws in S.weight_sets(dtype, p, ndim):
        what = f'rotation {ws.rotation}'
        arith = 'auto' if auto_ok and ws.rotation % 2 else 'bf16x2'
        pred = kom.LinearPredictor(ws.w, ws.b, p, ndim, arith=arith)
        assert pred.arith_for(TORCH[dtype]) == 'bf16x2'
        want_cells, decided = S.expected_cells(feats, ws, dtype, 'bf16x2')
        for k in ws.channels('sat') + ws.channels('const'):  # the condition of the spec, on this data
            assert decided[(slice(None),) * (ndim + 1) + (k,)].all(), f'{what} channel {k}'
        want_maps, dmaps = S.expected_maps(want_cells, decided, ndim, dims0)
        # the fused kernel's own predictions, read back from its maps
        lo, (maps, dims) = ns.encode(pred, enc, hi, padding=p)
        assert _last(kom) == _launch(family, 'encode'), what
        assert tuple(dims) == tuple(dims0) and np.array_equal(lo, ons.trim(ons.lowres_from_highres(padded), dims0))
        lines = S.mismatches(S.recover_predictions(gt, maps), want_maps, dmaps, ws)
        assert not lines, '\n'.join(lines)
        # the cell kernel
        cells, cells_f = pred.predict_cells(window, with_f32=True)
        assert _last(kom) == 'linear_bf16x2'
        bad = np.argwhere((cells != want_cells) & decided)
        assert bad.size == 0, (f'{what}: {len(bad)} cells, first {bad[:3].tolist()}: got '
                               f'{[int(cells[tuple(i)]) for i in bad[:3]]}, want {[int(want_cells[tuple(i)]) for i in bad[:3]]}, '
                               f'classes {[ws.cls[i[ndim + 1]][:2] for i in bad[:3]]}')
        assert np.array_equal(cells, cast_from_f32(cells_f, dtype)), f'{what}: cells are not the cast of their f32'
        # fused, generic and callable paths: the same bits, crossing channels included
        with kom._lib.option('KMP_DISABLE_LINEAR_FUSED', 1):
            lo_g, (maps_g, _) = ns.encode(pred, enc, hi, padding=p)
            assert _last(kom) == 'encode_generic'
        assert np.array_equal(lo_g, lo), what
        lines = S.mismatches(S.recover_predictions(gt, maps), S.recover_predictions(gt, maps_g),
                             [np.ones(m.shape, bool) for m in maps_g], ws)
        assert not lines and _same(maps, maps_g), f'{what}: fused != generic\n' + '\n'.join(lines)
        assert np.array_equal(ns.decode(pred, dec, lo_g, (maps_g, dims), padding=p), hi), f'{what}: generic -> own'
        called = ons.trim_maps([oenc(np.asarray(pm), g) for pm, g in zip(pred(window), gt_full)], dims0)
        assert _same(maps, called), f'{what}: fused != the coder on the callable\'s maps'
        lo_c, (maps_c, _) = ns.encode(lambda x: pred(x), enc, hi, padding=p)
        assert np.array_equal(lo_c, lo) and _same(maps_c, maps), f'{what}: callback encode'
        _decode_routes(kom, ns, pred, dec, lo, maps, dims, p, hi, family, chunk, what)


# ---------------------------------------------------------------------------------------------
# 32-bit samples: the f32 predictor on the generic path, the callable and the callback path
# ---------------------------------------------------------------------------------------------

WIDE = [(3, 0, (2, 9, 10, 12, 1)), (3, 1, (2, 9, 10, 12, 1)), (3, 0, (1, 8, 9, 7, 2)),
        (2, 0, (2, 17, 20, 1)), (2, 1, (2, 17, 20, 1)), (2, 2, (2, 17, 20, 1))]


@pytest.mark.parametrize('dtype', [I32, U32], ids=['int32', 'uint32'])
@pytest.mark.parametrize('ndim,p,shape', WIDE, ids=[f'p{c[1]}-{"x".join(map(str, c[2]))}' for c in WIDE])
def test_wide_sample_casts(kom, ndim, p, shape, dtype):
    ns, ons = (kom.volume, S.ons(3)) if ndim == 3 else (kom.image, S.ons(2))
    (enc, dec), (oenc, _) = S.coders(ns, dtype), S.coders(ons, dtype)
    hi = S.data(shape, dtype)
    _, _, window, feats = S.window_and_features(hi, p, ndim)
    chunk = S.split_chunk(shape, ndim)
    for ws in S.weight_sets_32(dtype, p, ndim):
        what = f'set {ws.rotation} {[c[1] for c in ws.cls]}'
        pred = kom.LinearPredictor(ws.w, ws.b, p, ndim, arith='f32')
        auto = kom.LinearPredictor(ws.w, ws.b, p, ndim)
        assert auto.arith_for(TORCH[dtype]) == 'f32'
        with np.errstate(invalid='ignore'):
            want_lo, (want_maps, want_dims) = ons.encode(OP.linear_predictions_fn(p, ws.w, ws.b, ndim), oenc, hi,
                                                         padding=p)
        exact = S.chain(feats, ws)
        want_cells = cast_from_f32(exact, dtype)
        for mfma in (0, 1):
            with kom._lib.option('KMP_LINEAR_F32_MFMA', mfma):
                cells, cells_f = pred.predict_cells(window, with_f32=True)
                assert _last(kom) == ('linear_mfma' if mfma else 'linear_valu')
            assert np.array_equal(cells_f.view(np.uint32), exact.view(np.uint32)), f'{what} mfma={mfma}'
            bad = np.argwhere(cells != want_cells)
            assert bad.size == 0, (f'{what} mfma={mfma}: {len(bad)} cells, first {bad[:3].tolist()}: got '
                                   f'{[int(cells[tuple(i)]) for i in bad[:3]]}, want '
                                   f'{[int(want_cells[tuple(i)]) for i in bad[:3]]}')
        for fn in (pred, auto, lambda x: pred(x)):
            lo, (maps, dims) = ns.encode(fn, enc, hi, padding=p)
            if fn is pred:
                assert _last(kom) == 'encode_generic'
            assert tuple(dims) == tuple(want_dims) and np.array_equal(lo, want_lo), what
            for i, (a, c) in enumerate(zip(maps, want_maps)):
                assert np.array_equal(a, c), f'{what} map {i}: {np.count_nonzero(np.asarray(a) != c)} mismatches'
        _decode_routes(kom, ns, pred, dec, lo, maps, dims, p, hi, 'generic', chunk, what)
    with pytest.raises(Exception):
        ns.encode(kom.LinearPredictor(ws.w, ws.b, p, ndim, arith='bf16x2'), enc, hi, padding=p)
