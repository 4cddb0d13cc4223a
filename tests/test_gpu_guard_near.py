"""Guard bands for the near-lossless coders: kmp_code, the four *_with_predictions* entry points and
the four fused calls with KMP_CODER_NEAR codes, on arenas the test owns (guard_spec.py, guard_capi.py)
at the three pointer-shift modes.  Per launch: guards, shift bytes and inputs untouched; unowned output
elements still the sentinel; owned ones bit-equal to tests/near_spec.py; two runs identical."""

import ctypes

import numpy as np
import pytest

import guard_capi as K
import guard_spec as G
from guard_capi import T
import near_spec as NS

pytestmark = pytest.mark.gpu

CODE = {np.dtype(np.uint8): 0, np.dtype(np.uint16): 1, np.dtype(np.int8): 5, np.dtype(np.int16): 6}
KMP_F32 = 3
DT_IDS = [np.dtype(d).name for d in NS.DTYPES]


def coder_arg(dtype, delta):
    return (4 if NS.width(dtype) == 8 else 5) | (delta << 8)


def bits(a):
    """An array as the unsigned array of its bit patterns (the arenas hold bytes)."""
    a = np.ascontiguousarray(a)
    return a.view(NS.map_dtype(a.dtype)) if a.dtype.kind == 'i' and a.dtype.itemsize < 4 else a


def named(prefix, arrays, role, masks=None):
    return [T(f'{prefix}{k}', role, bits(a), mask=None if masks is None else masks[f'{prefix}{k}'])
            for k, a in enumerate(arrays)]


def ptrs(p, tensors):
    return K.ptr_array([p[t.name] for t in tensors])


@pytest.mark.parametrize('dtype', NS.DTYPES, ids=DT_IDS)
def test_code(kom, dtype):
    code = CODE[np.dtype(dtype)]
    for n, delta in ((5, 1), (64, 3), (4099, NS.max_delta(dtype))):
        x = NS.noise((1, max(n, 12), 1), dtype, n).reshape(-1)[:n]
        pred = NS.noise((1, max(n, 12), 1), dtype, n + 1).reshape(-1)[::-1][:n]
        predf = NS.f32_predictions(max(n, 16), dtype, seed=n)[:n]
        coder = coder_arg(dtype, delta)
        for pd, pcode in ((pred, code), (predf, KMP_F32)):
            enc = NS.encode_values(pd, x, delta)
            dec = NS.decode_values(pd, enc, delta, dtype)
            for shift in K.SHIFTS:
                name = K.launch('kmp_code', [T('pred', 'in', bits(pd)), T('x', 'in', bits(x)), T('out', 'out', enc)],
                                lambda fn, q: fn(0, coder, pcode, q['pred'], code, q['x'], n, q['out'], None), shift)
                assert name == 'code'
                name = K.launch('kmp_code', [T('pred', 'in', bits(pd)), T('x', 'in', enc), T('out', 'out', bits(dec))],
                                lambda fn, q: fn(1, coder, pcode, q['pred'], code, q['x'], n, q['out'], None), shift)
                assert name == 'code'


@pytest.mark.parametrize('dtype', NS.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize('shape', [(2, 5, 6, 17, 1), (1, 5, 6, 7, 3), (3, 7, 33, 1), (2, 8, 9, 2)],
                         ids=['5x6x17', '5x6x7c3', '7x33', '8x9c2'])
def test_encode_decode_with_predictions(kom, dtype, shape):
    """The four coder launches around predictions_fn: prediction maps of the sample dtype (plain and
    _typed) and float32 (_typed), full-range noise for samples and predictions."""
    nsp = len(shape) - 2
    o = NS.ons(nsp)
    code = CODE[np.dtype(dtype)]
    delta = 3 if shape[-1] == 1 else NS.max_delta(dtype)
    coder = coder_arg(dtype, delta)
    x = NS.noise(shape, dtype, seed=shape[-2])
    sp, C = shape[1:1 + nsp], shape[-1]
    hp, dims = o.pad_highres(x)
    lowres_p, gt = o.lowres_from_highres(hp), o.maps_from_highres(hp)
    lo = np.ascontiguousarray(o.trim(lowres_p, dims))
    for pdt, entries in ((dtype, ('', '_typed')), (np.float32, ('_typed',))):
        if pdt == np.float32:
            preds = [NS.f32_predictions(g.size, dtype, seed=60 + k).reshape(g.shape) for k, g in enumerate(gt)]
        else:
            preds = [NS.noise((1, g.size, 1), dtype, 50 + k).reshape(g.shape) for k, g in enumerate(gt)]
        coded = [np.ascontiguousarray(m) for m in
                 o.trim_maps([NS.encode_values(q, g, delta) for q, g in zip(preds, gt)], dims)]
        back = np.ascontiguousarray(o.trim(o.highres_from_lowres_and_maps(
            o.pad_lowres(lo, tuple(dims)),
            [NS.decode_values(q, e, delta, dtype) for q, e in zip(preds, o.pad_maps(coded, tuple(dims)))]), dims))
        assert np.abs(back.astype(np.int64) - x.astype(np.int64)).max() <= delta
        pin = named('pred', preds, 'in')
        pcode = KMP_F32 if pdt == np.float32 else code
        for suffix in entries:
            typed = (pcode,) if suffix else ()
            for shift in K.SHIFTS:
                mout = named('map', coded, 'out')
                name = K.launch('kmp_encode_with_predictions' + suffix,
                                [T('highres', 'in', bits(x))] + pin + [T('lowres', 'out', bits(lo))] + mout,
                                lambda fn, q: fn(nsp, code, coder, *typed, q['highres'], shape[0], K.i64x3(sp), C,
                                                 ptrs(q, pin), q['lowres'], ptrs(q, mout), None), shift)
                assert name == 'encode_with_predictions'
                min_ = named('map', coded, 'in')
                name = K.launch('kmp_decode_with_predictions' + suffix,
                                [T('lowres', 'in', bits(lo))] + min_ + pin + [T('highres', 'out', bits(back))],
                                lambda fn, q: fn(nsp, code, coder, *typed, q['lowres'], ptrs(q, min_), shape[0],
                                                 K.i64x3(lo.shape[1:1 + nsp]), C, K.i32x3(dims), ptrs(q, pin),
                                                 q['highres'], None), shift)
                assert name == 'decode_with_predictions'


FUSED = [((2, 5, 6, 17, 1), 'mean', 1), ((2, 6, 5, 9, 1), 'linear', 0), ((1, 5, 6, 7, 3), 'mean', 0),
         ((3, 7, 33, 1), 'linear', 1), ((3, 7, 16, 1), 'mean', 2), ((2, 7, 9, 3), 'linear', 0)]


@pytest.mark.parametrize('dtype', NS.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize('shape,kind,p', FUSED, ids=[f'{"x".join(map(str, s[1:]))}-{k}-p{p}' for s, k, p in FUSED])
def test_fused_calls(kom, dtype, shape, kind, p):
    """kmp_volume_* / kmp_image_* with a near code: the generic family, the whole frame and a box."""
    from kompressor_amd import _lib
    nsp = len(shape) - 2
    code = CODE[np.dtype(dtype)]
    delta = 2 if kind == 'mean' else NS.max_delta(dtype)
    coder = coder_arg(dtype, delta)
    x = NS.noise(shape, dtype, seed=sum(shape))
    if kind == 'mean':
        fn, w, b = NS.mean_fn(p, nsp, dtype), None, None
    else:
        w, b = NS.linear_weights(p, nsp)
        fn = NS.linear_fn(p, w, b, nsp, dtype)
    lo, maps, dims = NS.encode_level(x, fn, nsp, p, delta)
    rec = NS.decode_level(lo, maps, dims, fn, nsp, p, delta)
    sp, C, E = shape[1:1 + nsp], shape[-1], lo.shape[1:1 + nsp]
    wt = [] if w is None else [T('weights', 'in', w), T('bias', 'in', b)]

    def pstruct(q):
        return _lib.Predictor(0 if w is None else 1, p, q.get('weights'), q.get('bias'))

    probe = _lib.Predictor(0 if w is None else 1, p, None, None)
    wsb = _lib.lib.kmp_volume_workspace_bytes if nsp == 3 else _lib.lib.kmp_image_workspace_bytes
    need = int(wsb(code, shape[0], *sp, C, ctypes.byref(probe)))
    ws = T('workspace', 'scratch', np.zeros((max(need, 1),), np.uint8), align=256)  # holds sample-dtype cells
    enc_entry, dec_entry = ('kmp_volume_encode', 'kmp_volume_decode') if nsp == 3 else ('kmp_image_encode',
                                                                                       'kmp_image_decode')
    box = [(1, e) if a % 2 == 0 else (0, max(e - 1, 1)) for a, e in enumerate(E)]
    for region, shift in ((None, 'none'), (None, 'all'), (None, 'out'), (box, 'all')):
        reg = None
        if region is not None:
            reg = _lib.Region()
            for a in range(3):
                reg.begin[a], reg.end[a] = (0, 1) if a < 3 - nsp else region[a - (3 - nsp)]
        regp = ctypes.byref(reg) if reg is not None else None
        em = G.encode_masks(lo.shape, [m.shape for m in maps], region, nsp)
        mout = named('map', maps, 'out', em)
        dims_out = (ctypes.c_int32 * 3)()
        name = K.launch(enc_entry, [T('highres', 'in', bits(x))] + wt + [T('lowres', 'out', bits(lo), mask=em['lowres'])]
                        + mout + [ws],
                        lambda fn_, q: fn_(code, q['highres'], shape[0], *sp, C, ctypes.byref(pstruct(q)), coder,
                                           q['lowres'], ptrs(q, mout), dims_out, regp, q['workspace'], need, None),
                        shift)
        assert name == 'encode_generic' and tuple(dims_out[:nsp]) == dims
        min_ = named('map', maps, 'in')
        dm = G.decode_masks(x.shape, lo.shape, region, nsp)['highres']
        name = K.launch(dec_entry, [T('lowres', 'in', bits(lo))] + min_ + wt + [T('highres', 'out', bits(rec), mask=dm), ws],
                        lambda fn_, q: fn_(code, q['lowres'], ptrs(q, min_), shape[0], *E, C, K.i32x3(dims),
                                           ctypes.byref(pstruct(q)), coder, q['highres'], regp, q['workspace'], need,
                                           None), shift)
        assert name == 'decode_generic'
