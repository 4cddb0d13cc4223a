"""Guard bands for signed samples: the fused families that take int8 / int16 (wave3d, wave2d, generic)
and the non-fused C-ABI launches with KMP_I8 / KMP_I16, on arenas the test owns (guard_spec.py,
guard_capi.py).  Per launch: guards, pointer shifts and inputs untouched; nothing outside the region's
box written; the box bit-equal to tests/signed_spec.py; two runs on two sentinel fills identical; and
the launch's name."""

import numpy as np
import pytest
import torch

from oracle.common import cast_from_f32
from oracle import predictors as OP
import guard_spec as G
import guard_capi as K
from guard_capi import T
import signed_spec as S
from test_gpu_signed import ROW_BY_ID, NP2T, reference, _predictor, _coders, _launch_name, _weights

pytestmark = pytest.mark.gpu

I8, I16 = np.int8, np.int16
KMP_I8, KMP_I16, KMP_F32 = 5, 6, 3
CODE = {np.dtype(I8): KMP_I8, np.dtype(I16): KMP_I16}
CODER = {np.dtype(I8): 1, np.dtype(I16): 2}

FUSED = [('vol-p0', I16), ('vol-p0', I8), ('vol-p0-odd', I16), ('vol-p0-odd', I8), ('img-p0', I16), ('img-p0', I8),
         ('img-p0-odd', I16), ('img-p0-odd', I8), ('vol-c3', I16), ('vol-w48-p1', I8), ('vol-lin-p0', I16),
         ('vol-lin-p1', I8), ('img-lin-p0', I16), ('img-lin-p0-wave', I16)]


def _bits(a):
    """A signed array as the unsigned array of its bit patterns (the arenas hold bytes)."""
    a = np.ascontiguousarray(a)
    return a.view(S.unsigned_of(a.dtype)) if a.dtype in (np.int8, np.int16) else a


def run_fused(kom, rid, dtype, region):
    from kompressor_amd import _nd, _lib
    _, shape, _, kind, p, family = ROW_BY_ID[rid]
    ndim = len(shape) - 2
    ns = kom.volume if ndim == 3 else kom.image
    enc, dec = _coders(ns, dtype)
    ref = reference(rid, dtype)
    x, lo, maps, dims = ref['x'], ref['lowres'], ref['maps'], ref['dims']
    pred = _predictor(kom, kind, p, ndim)
    td = NP2T[np.dtype(dtype)]
    tu = {1: torch.uint8, 2: torch.uint16}[np.dtype(dtype).itemsize]
    last = lambda: kom._lib.lib.kmp_last_launch().decode()  # noqa: E731
    outs = {'lowres': lo, **{f'map{k}': m for k, m in enumerate(maps)}}
    tdt = {'highres': td, 'lowres': td, **{f'map{k}': tu for k in range(len(maps))}}

    def carve(arr, name, s, filled):
        c = G.carve_arena(arr.shape, tdt[name], 'cuda', s)
        return G.fill(c, arr) if filled else c

    plan = _nd.fused_plan(pred, enc, p, td, ndim, _lib.ENCODE)
    assert plan is not None

    def run_encode(s):
        t = {'highres': carve(x, 'highres', s, True)}
        t.update({name: carve(a, name, s, False) for name, a in outs.items()})
        need = _nd.workspace_bytes(t['highres'].payload, pred, ndim)
        t['workspace'] = G.carve_arena((need,), torch.uint8, 'cuda', s)
        got = _nd.fused_encode_into(t['highres'].payload, plan[0], plan[1], t['lowres'].payload,
                                    [t[f'map{k}'].payload for k in range(len(maps))], ndim, region=region,
                                    workspace=t['workspace'].payload)
        assert tuple(got) == dims
        assert last() == _launch_name(family, 'encode')
        return t

    G.check_launch_pair(run_encode, {'highres': x}, list(outs), outs,
                        G.encode_masks(lo.shape, [m.shape for m in maps], region, ndim))

    plan = _nd.fused_plan(pred, dec, p, td, ndim, _lib.DECODE)
    assert plan is not None

    def run_decode(s):
        t = {name: carve(a, name, s, True) for name, a in outs.items()}
        t['highres'] = carve(x, 'highres', s, False)
        need = _nd.workspace_bytes(t['highres'].payload, pred, ndim)
        t['workspace'] = G.carve_arena((need,), torch.uint8, 'cuda', s)
        _nd.fused_decode_into(t['lowres'].payload, [t[f'map{k}'].payload for k in range(len(maps))], dims, plan[0],
                              plan[1], t['highres'].payload, ndim, region=region, workspace=t['workspace'].payload)
        assert last() == _launch_name(family, 'decode')
        return t

    G.check_launch_pair(run_decode, outs, ['highres'], {'highres': x}, G.decode_masks(x.shape, lo.shape, region, ndim))


@pytest.mark.parametrize('rid,dtype', FUSED, ids=[f'{r}-{np.dtype(d).name}' for r, d in FUSED])
def test_fused_guards_regions_and_determinism(kom, rid, dtype):
    """The whole frame, then a region of the leading spatial axis (z slabs of a volume, rows of an image:
    the one-pass families keep it) strictly inside and touching the end."""
    ref = reference(rid, dtype)
    ndim = ref['x'].ndim - 2
    E = ref['lowres'].shape[1:1 + ndim]
    rest = [(0, int(e)) for e in E[1:]]
    for region in (None, [(1, E[0] - 1)] + rest, [(E[0] // 2, E[0])] + rest):
        run_fused(kom, rid, dtype, region)


# ---------------------------------------------------------------------------------------------
# the non-fused entry points with the signed dtype codes
# ---------------------------------------------------------------------------------------------

def _named(prefix, arrays, role):
    return [T(f'{prefix}{k}', role, _bits(a)) for k, a in enumerate(arrays)]


def _ptrs(p, tensors):
    return K.ptr_array([p[t.name] for t in tensors])


@pytest.mark.parametrize('dtype', [I16, I8], ids=['int16', 'int8'])
@pytest.mark.parametrize('shape,pads', [((2, 5, 6, 9, 1), (0, 1)), ((2, 5, 6, 17, 1), (0,)), ((1, 5, 6, 7, 2), (0, 1)),
                                        ((3, 9, 19, 1), (0, 1, 2))], ids=['5x6x9', '5x6x17', '5x6x7c2', '9x19'])
def test_mean_predict_maps(kom, dtype, shape, pads):
    nsp = len(shape) - 2
    code = CODE[np.dtype(dtype)]
    for p in pads:
        window = S.ons(nsp).pad_neighborhood(S.data(shape, dtype, seed=p + shape[-2]), p)
        Sx = window.shape[1:1 + nsp]
        maps = S.predictions(window, S.mean_fn(p, nsp))
        for entry, typed in (('kmp_mean_predict_maps', ()), ('kmp_mean_predict_maps_typed', (code,))):
            for shift in K.SHIFTS:
                outs = _named('map', maps, 'out')
                name = K.launch(entry, [T('window', 'in', _bits(window))] + outs,
                                lambda fn, q: fn(nsp, code, *typed, q['window'], shape[0], K.i64x3(Sx), shape[-1], p,
                                                 _ptrs(q, outs), None), shift)
                assert name == 'mean_predict_maps'


@pytest.mark.parametrize('dtype', [I16, I8], ids=['int16', 'int8'])
@pytest.mark.parametrize('mfma', [0, 1], ids=['valu', 'f32mfma'])
@pytest.mark.parametrize('nsp,cells,pads', [(3, (3, 4, 6), (0, 1)), (3, (2, 3, 17), (0,)), (2, (3, 17), (0, 1, 2))],
                         ids=['3x4x6', '2x3x17', '3x17'])
def test_linear_predict(kom, kmp_opt, dtype, mfma, nsp, cells, pads):
    """Both float32 kernels: M^-1 of the cast (in the mapped domain) of the oracle's fma chain over
    M(window); the float32 cells are the chain's own values."""
    kmp_opt('KMP_LINEAR_F32_MFMA', mfma)
    code = CODE[np.dtype(dtype)]
    u = S.unsigned_of(dtype)
    for p in pads:
        window = S.data((2, *[c + 2 * p + 1 for c in cells], 1), dtype, seed=7 * p + cells[-1])
        w, b = _weights(p, nsp)
        exact = OP.linear_fma_chain(S.ons(nsp).features_from_lowres(S.M(window), p), w, b)
        want = S.Minv(cast_from_f32(exact, u))
        Sx = window.shape[1:1 + nsp]
        for f32 in (True, False):
            for shift in K.SHIFTS:
                ts = [T('window', 'in', _bits(window)), T('weights', 'in', w), T('bias', 'in', b),
                      T('preds', 'out', _bits(want))]
                if f32:
                    ts.append(T('preds_f32', 'out', exact))
                name = K.launch('kmp_linear_predict', ts,
                                lambda fn, q: fn(nsp, code, q['window'], window.shape[0], K.i64x3(Sx), 1, p, q['weights'],
                                                 q['bias'], q['preds'], q['preds_f32'] if f32 else None, None), shift)
                assert name == ('linear_mfma' if mfma else 'linear_valu')


@pytest.mark.parametrize('dtype', [I16, I8], ids=['int16', 'int8'])
def test_code(kom, dtype):
    """kmp_code with the signed code for both operands, and float32 predictions against signed samples."""
    code, coder = CODE[np.dtype(dtype)], CODER[np.dtype(dtype)]
    for n in (5, 64, 4099):
        gt, pred = S.uniform((n,), dtype, n), S.uniform((n,), dtype, n + 1)
        gt[:5], pred[:5] = S.extremes(dtype), S.extremes(dtype)[::-1]
        predf = (pred.astype(np.float64) + np.random.default_rng(n).uniform(-0.999, 0.999, n)).astype(np.float32)
        for pd, pcode, pi in ((pred, code, pred.astype(np.int64)), (predf, KMP_F32, cast_from_f32(predf, np.int32))):
            enc = S.encode_values(pi, gt)
            assert np.array_equal(S.decode_values(pi, enc, dtype), gt)
            for shift in K.SHIFTS:
                name = K.launch('kmp_code', [T('pred', 'in', _bits(pd)), T('x', 'in', _bits(gt)), T('out', 'out', enc)],
                                lambda fn, q: fn(0, coder, pcode, q['pred'], code, q['x'], n, q['out'], None), shift)
                assert name == 'code'
                # decode: x is the encoded map (the coder's unsigned type), the output the sample bits
                ecode = {1: 0, 2: 1}[np.dtype(dtype).itemsize]
                name = K.launch('kmp_code', [T('pred', 'in', _bits(pd)), T('x', 'in', enc), T('out', 'out', _bits(gt))],
                                lambda fn, q: fn(1, coder, pcode, q['pred'], ecode, q['x'], n, q['out'], None), shift)
                assert name == 'code'


@pytest.mark.parametrize('form', ['rows', 'elements'])
@pytest.mark.parametrize('dtype', [I16, I8], ids=['int16', 'int8'])
@pytest.mark.parametrize('shape', [(2, 5, 6, 17, 1), (2, 6, 5, 15, 1), (1, 5, 6, 7, 3), (3, 7, 33, 1)],
                         ids=['5x6x17', '6x5x15', '5x6x7c3', '7x33'])
def test_encode_decode_with_predictions(kom, kmp_opt, form, dtype, shape):
    """The four coder launches around predictions_fn with the signed code: prediction maps of the sample
    dtype (plain and _typed) and float32 (_typed), both kernel forms."""
    kmp_opt('KMP_DISABLE_ROWS', 1 if form == 'elements' else None)
    nsp = len(shape) - 2
    o = S.ons(nsp)
    code, coder = CODE[np.dtype(dtype)], CODER[np.dtype(dtype)]
    x = S.data(shape, dtype, seed=shape[-2])
    sp, C = shape[1:1 + nsp], shape[-1]
    hp, dims = o.pad_highres(x)
    lowres_p, gt = o.lowres_from_highres(hp), o.maps_from_highres(hp)
    lo = np.ascontiguousarray(o.trim(lowres_p, dims))
    for pdt, entries in ((dtype, ('', '_typed')), (np.float32, ('_typed',))):
        preds = []
        for k, g in enumerate(gt):
            ints = S.uniform(g.shape, dtype, 50 + k)
            if pdt == np.float32:
                frac = np.random.default_rng(60 + k).uniform(-0.999, 0.999, g.shape)
                preds.append((ints.astype(np.float64) + frac).astype(np.float32))
            else:
                preds.append(ints)
        as_int = [cast_from_f32(q, np.int32) if pdt == np.float32 else q for q in preds]
        coded = [np.ascontiguousarray(m) for m in o.trim_maps([S.encode_values(q, g) for q, g in zip(as_int, gt)], dims)]
        back = o.trim(o.highres_from_lowres_and_maps(
            o.pad_lowres(lo, tuple(dims)),
            [S.decode_values(q, e, dtype) for q, e in zip(as_int, o.pad_maps(coded, tuple(dims)))]), dims)
        assert np.array_equal(back, x)
        pin = _named('pred', preds, 'in')
        pcode = KMP_F32 if pdt == np.float32 else code
        for suffix in entries:
            typed = (pcode,) if suffix else ()
            for shift in K.SHIFTS:
                mout = _named('map', coded, 'out')
                name = K.launch('kmp_encode_with_predictions' + suffix,
                                [T('highres', 'in', _bits(x))] + pin + [T('lowres', 'out', _bits(lo))] + mout,
                                lambda fn, q: fn(nsp, code, coder, *typed, q['highres'], shape[0], K.i64x3(sp), C,
                                                 _ptrs(q, pin), q['lowres'], _ptrs(q, mout), None), shift)
                assert name == 'encode_with_predictions'
                min_ = _named('map', coded, 'in')
                name = K.launch('kmp_decode_with_predictions' + suffix,
                                [T('lowres', 'in', _bits(lo))] + min_ + pin + [T('highres', 'out', _bits(x))],
                                lambda fn, q: fn(nsp, code, coder, *typed, q['lowres'], _ptrs(q, min_), shape[0],
                                                 K.i64x3(lo.shape[1:1 + nsp]), C, K.i32x3(dims), _ptrs(q, pin),
                                                 q['highres'], None), shift)
                assert name == 'decode_with_predictions'
