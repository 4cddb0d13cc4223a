"""Guard bands, exact ownership and off-alignment pointers for the callback path -- the steps a
trained network as ``predictions_fn`` runs between (kmp_callback.hip: the window gathers and the coder
launches around the callback) -- and for the predictor primitives a built-in predictions_fn is made of
(mean_predict_maps, maps_from_predictions, linear_predict), called through ``kompressor_amd._lib.lib``
with every tensor, each of the 7 (3) maps included, in a sentinel-filled arena of its own
(guard_capi.py).  Checks, shifts and row lengths as in test_gpu_guard_primitives.py; expected values
from the numpy oracle alone.

``kmp_linear_predict_mfma`` is not bit-equal to the oracle by design: its float32 cells are held to
1e-5 * (sum |f w| + |b|) around the float64 value of the bf16x2 split, its integer cells to the cast of
its own float32 cells (or, without a float32 output, to the casts of that interval's ends)."""

import numpy as np
import pytest

from oracle import common as OC
from oracle import predictors as OP
import guard_capi as K
from guard_capi import T, CODE, DTYPES, DT_IDS, shapes, ons, form  # noqa: F401  (form: a fixture)

pytestmark = pytest.mark.gpu

LAUNCHES = ('kmp_window_from_highres', 'kmp_window_from_lowres', 'kmp_encode_with_predictions',
            'kmp_decode_with_predictions', 'kmp_encode_with_predictions_typed', 'kmp_decode_with_predictions_typed',
            'kmp_mean_predict_maps', 'kmp_mean_predict_maps_typed', 'kmp_maps_from_predictions',
            'kmp_linear_predict', 'kmp_linear_predict_mfma')

NMAPS = {3: 7, 2: 3}
CODER_OF = {np.dtype(np.uint8): (1, 'uint8'), np.dtype(np.uint16): (2, 'uint16'), np.dtype(np.int32): (0, 'raw')}


def _named(prefix, arrays, role):
    return [T(f'{prefix}{k}', role, a) for k, a in enumerate(arrays)]


def _ptrs(p, tensors):
    return K.ptr_array([p[t.name] for t in tensors])


# ---------------------------------------------------------------------------------------------
# the window gathers
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize('p', [0, 1, 2])
@pytest.mark.parametrize('nsp', [3, 2])
@pytest.mark.parametrize('dtype', DTYPES[:4], ids=DT_IDS[:4])
def test_windows(kom, form, dtype, nsp, p):
    """The windows encode (from the highres) and decode (from the trimmed lowres and ``dims``) hand
    predictions_fn, against the oracle's composition of pad_highres / lowres_from_highres / pad_lowres /
    pad_neighborhood."""
    code = CODE[np.dtype(dtype)]
    o = ons(nsp)
    for shape in shapes(dtype, nsp):
        x = K.rand(shape, dtype, shape[-2] + 5 * p)
        sp, C = shape[1:1 + nsp], shape[-1]
        hp, dims = o.pad_highres(x)
        lowres = o.lowres_from_highres(hp)
        want = o.pad_neighborhood(lowres, p)
        lo = np.ascontiguousarray(o.trim(lowres, dims))
        want_lo = o.pad_neighborhood(o.pad_lowres(lo, tuple(dims)), p)
        assert want.shape == want_lo.shape
        for shift in K.SHIFTS:
            name = K.launch('kmp_window_from_highres', [T('highres', 'in', x), T('window', 'out', want)],
                            lambda fn, q: fn(nsp, code, q['highres'], shape[0], K.i64x3(sp), C, p, q['window'], None),
                            shift)
            assert name == 'window'
            name = K.launch('kmp_window_from_lowres', [T('lowres', 'in', lo), T('window', 'out', want_lo)],
                            lambda fn, q: fn(nsp, code, q['lowres'], shape[0], K.i64x3(lo.shape[1:1 + nsp]), C,
                                             K.i32x3(dims), p, q['window'], None), shift)
            assert name == 'window'


# ---------------------------------------------------------------------------------------------
# the coder launches on either side of predictions_fn
# ---------------------------------------------------------------------------------------------

def _pred_maps(gt_maps, dtype, pdt, seed):
    """Random full-range prediction maps in the untrimmed map shapes: of the sample dtype, or float32
    values over the same range with fractions (what a network emits)."""
    out = []
    for k, g in enumerate(gt_maps):
        ints = K.rand(g.shape, dtype, seed + k)
        if pdt == np.float32:
            frac = np.random.default_rng(seed + 100 + k).uniform(-0.999, 0.999, g.shape)
            out.append((ints.astype(np.float64) + frac).astype(np.float32))
        else:
            out.append(ints)
    return out


@pytest.mark.parametrize('nsp', [3, 2])
@pytest.mark.parametrize('dtype', [np.uint8, np.uint16, np.int32], ids=['uint8', 'uint16', 'int32'])
def test_encode_decode_with_predictions(kom, form, dtype, nsp):
    """u8 / u16 with their coders, int32 with RAW; prediction maps of the sample dtype (the plain and
    the _typed entry point) and float32 (_typed).  Expected: the oracle's maps_from_highres, the
    oracle.common coder per map, and the trims."""
    code = CODE[np.dtype(dtype)]
    coder, cname = CODER_OF[np.dtype(dtype)]
    enc, dec = getattr(OC, 'encode_values_' + cname), getattr(OC, 'decode_values_' + cname)
    o = ons(nsp)
    for shape in shapes(dtype, nsp):
        x = K.rand(shape, dtype, shape[-2] + 11)
        sp, C = shape[1:1 + nsp], shape[-1]
        hp, dims = o.pad_highres(x)
        o.validate_highres(hp)
        lowres_p, gt = o.lowres_from_highres(hp), o.maps_from_highres(hp)
        o.validate_lowres(lowres_p)
        lo = np.ascontiguousarray(o.trim(lowres_p, dims))
        for pdt, entries in ((dtype, ('', '_typed')), (np.float32, ('_typed',))):
            preds = _pred_maps(gt, dtype, pdt, shape[-2])
            coded = [np.ascontiguousarray(m) for m in o.trim_maps([enc(q, g) for q, g in zip(preds, gt)], dims)]
            back = o.trim(o.highres_from_lowres_and_maps(
                o.pad_lowres(lo, tuple(dims)), [dec(q, e) for q, e in zip(preds, o.pad_maps(coded, tuple(dims)))]), dims)
            assert np.array_equal(back, x)
            pin = _named('pred', preds, 'in')
            for suffix in entries:
                typed = (CODE[np.dtype(pdt)],) if suffix else ()
                for shift in K.SHIFTS:
                    mout = _named('map', coded, 'out')
                    name = K.launch(
                        'kmp_encode_with_predictions' + suffix,
                        [T('highres', 'in', x)] + pin + [T('lowres', 'out', lo)] + mout,
                        lambda fn, q: fn(nsp, code, coder, *typed, q['highres'], shape[0], K.i64x3(sp), C,
                                         _ptrs(q, pin), q['lowres'], _ptrs(q, mout), None), shift)
                    assert name == 'encode_with_predictions'
                    min_ = _named('map', coded, 'in')
                    name = K.launch(
                        'kmp_decode_with_predictions' + suffix,
                        [T('lowres', 'in', lo)] + min_ + pin + [T('highres', 'out', x)],
                        lambda fn, q: fn(nsp, code, coder, *typed, q['lowres'], _ptrs(q, min_), shape[0],
                                         K.i64x3(lo.shape[1:1 + nsp]), C, K.i32x3(dims), _ptrs(q, pin), q['highres'],
                                         None), shift)
                    assert name == 'decode_with_predictions'


# ---------------------------------------------------------------------------------------------
# the mean predictor
# ---------------------------------------------------------------------------------------------

# (lowres shape before the neighbourhood padding, paddings, launch name at C == 1 rows)
MEAN_WINDOWS = [
    ((2, 5, 6, 9, 1), (0,), 'mean_predict_p0x8'), ((2, 5, 6, 17, 1), (0,), 'mean_predict_p0x8'),
    ((3, 5, 6, 10, 1), (0, 1, 2), 'mean_predict_plane'), ((2, 7, 8, 21, 1), (0, 1, 2), 'mean_predict_plane'),
    ((3, 9, 10, 1), (0, 1, 2), 'mean_predict_maps'), ((3, 9, 19, 1), (0, 1, 2), 'mean_predict_maps'),
]


@pytest.mark.parametrize('dtype', [np.uint8, np.uint16], ids=['uint8', 'uint16'])
@pytest.mark.parametrize('case', MEAN_WINDOWS, ids=['x'.join(map(str, c[0])) for c in MEAN_WINDOWS])
def test_mean_predict_maps(kom, form, dtype, case):
    """The window is the listed lowres padded by p.  Cells x % 8 == 0 at p = 0 takes the eight-per-lane
    kernel, the other volumes the plane kernel (whose loads cover the byte range in aligned 16-byte
    blocks), images the row kernels.  Maps in the sample dtype (both entry points) and, for volumes, in
    float32: the same integers."""
    shape, pads, family = case
    nsp = len(shape) - 2
    code = CODE[np.dtype(dtype)]
    for p in pads:
        window = ons(nsp).pad_neighborhood(K.rand(shape, dtype, shape[-2] + p), p)
        S = window.shape[1:1 + nsp]
        maps = [np.ascontiguousarray(m) for m in OP.mean_predictions_fn(p, nsp)(window)]
        assert len(maps) == NMAPS[nsp] and all(m.dtype == np.dtype(dtype) for m in maps)
        variants = [('kmp_mean_predict_maps', (), maps), ('kmp_mean_predict_maps_typed', (code,), maps)]
        if nsp == 3:
            variants.append(('kmp_mean_predict_maps_typed', (CODE[np.dtype(np.float32)],),
                             [m.astype(np.float32) for m in maps]))
        for entry, typed, want in variants:
            for shift in K.SHIFTS:
                outs = _named('map', want, 'out')
                name = K.launch(entry, [T('window', 'in', window)] + outs,
                                lambda fn, q: fn(nsp, code, *typed, q['window'], shape[0], K.i64x3(S), 1, p,
                                                 _ptrs(q, outs), None), shift)
                assert name.startswith(family), (name, family)


# (dtype, channel counts) no LDS kernel serves: the cell means, then the per-element aggregation of them
MEAN_ELEMENT = [(np.int32, (1, 2)), (np.uint32, (1, 2)), (np.uint8, (2,)), (np.uint16, (2,))]


@pytest.mark.parametrize('nsp', [3, 2])
@pytest.mark.parametrize('dtype,channels', MEAN_ELEMENT, ids=[np.dtype(d).name for d, _ in MEAN_ELEMENT])
def test_mean_predict_maps_elements(kom, form, dtype, channels, nsp):
    """The two-pass element fallback (cell_mean_map_kernel, then the cell-means form of the element
    aggregation in its general <T, I> instantiation) on full-range samples: 32-bit samples at C == 1 and
    C == 2, u8 / u16 at C == 2, maps of the sample dtype through both entry points."""
    code = CODE[np.dtype(dtype)]
    for C in channels:
        shape = (2, 5, 6, 7, C) if nsp == 3 else (3, 7, 9, C)
        for p in (0, 1, 2):
            window = ons(nsp).pad_neighborhood(K.rand(shape, dtype, shape[-2] + 3 * p + C), p)
            S = window.shape[1:1 + nsp]
            maps = [np.ascontiguousarray(m) for m in OP.mean_predictions_fn(p, nsp)(window)]
            assert len(maps) == NMAPS[nsp] and all(m.dtype == np.dtype(dtype) for m in maps)
            for entry, typed in (('kmp_mean_predict_maps', ()), ('kmp_mean_predict_maps_typed', (code,))):
                for shift in K.SHIFTS:
                    outs = _named('map', maps, 'out')
                    name = K.launch(entry, [T('window', 'in', window)] + outs,
                                    lambda fn, q: fn(nsp, code, *typed, q['window'], shape[0], K.i64x3(S), C, p,
                                                     _ptrs(q, outs), None), shift)
                    assert name == 'mean_predict_maps'


# ---------------------------------------------------------------------------------------------
# maps_from_predictions
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize('nsp', [3, 2])
@pytest.mark.parametrize('dtype', DTYPES[:4], ids=DT_IDS[:4])
def test_maps_from_predictions(kom, form, dtype, nsp):
    code = CODE[np.dtype(dtype)]
    Kp = 19 if nsp == 3 else 5
    for w in (1, 7, 63, 64, 65):
        for C in (1, 2) if w == 7 else (1,):
            cells = (2, 3, 5, w) if nsp == 3 else (2, 5, w)
            preds = K.rand((*cells, Kp, C), dtype, w + C)
            maps = [np.ascontiguousarray(m) for m in ons(nsp).maps_from_predictions(preds)]
            for shift in K.SHIFTS:
                outs = _named('map', maps, 'out')
                name = K.launch('kmp_maps_from_predictions', [T('preds', 'in', preds)] + outs,
                                lambda fn, q: fn(nsp, code, q['preds'], cells[0], K.i64x3(cells[1:]), C, _ptrs(q, outs),
                                                 None), shift)
                assert name == 'maps_from_predictions'


# ---------------------------------------------------------------------------------------------
# the linear predictor's cells
# ---------------------------------------------------------------------------------------------

def _weights(nsp, p, seed, dtype):
    n, k = (2 * p + 2) ** nsp, 19 if nsp == 3 else 5
    rng = np.random.default_rng(seed)
    w = (1.0 / n + rng.standard_normal((n, k)) * (0.3 / n)).astype(np.float32)  # a noisy mean
    b = (rng.standard_normal(k) * (3.0 if dtype == np.uint8 else 50.0)).astype(np.float32)
    return w, b


LINEAR = [(3, (3, 4, 6), (0, 1)), (3, (2, 3, 17), (0, 1)), (2, (4, 6), (0, 1, 2)), (2, (3, 17), (0, 1, 2))]


def _linear_case(nsp, cells, p, dtype):
    window = K.rand((2, *[c + 2 * p + 1 for c in cells], 1), dtype, 7 * p + cells[-1])
    w, b = _weights(nsp, p, 2 + p, dtype)
    return window, w, b, ons(nsp).features_from_lowres(window, p)


def _linear_call(nsp, code, window, p, f32):
    S = window.shape[1:1 + nsp]
    return lambda fn, q: fn(nsp, code, q['window'], window.shape[0], K.i64x3(S), 1, p, q['weights'], q['bias'],
                            q['preds'], q['preds_f32'] if f32 else None, None)


@pytest.mark.parametrize('mfma', [0, 1], ids=['valu', 'f32mfma'])
@pytest.mark.parametrize('dtype', [np.uint8, np.uint16], ids=['uint8', 'uint16'])
@pytest.mark.parametrize('case', LINEAR, ids=['x'.join(map(str, c[1])) for c in LINEAR])
def test_linear_predict(kom, kmp_opt, dtype, case, mfma):
    """Both float32 kernels are the oracle's k-ordered fma chain bit for bit, with the float32 cells
    asked for and not (NULL)."""
    nsp, cells, pads = case
    kmp_opt('KMP_LINEAR_F32_MFMA', mfma)
    code = CODE[np.dtype(dtype)]
    for p in pads:
        window, w, b, feats = _linear_case(nsp, cells, p, dtype)
        exact = OP.linear_fma_chain(feats, w, b)
        want = OC.cast_from_f32(exact, dtype)
        for f32 in (True, False):
            for shift in K.SHIFTS:
                ts = [T('window', 'in', window), T('weights', 'in', w), T('bias', 'in', b), T('preds', 'out', want)]
                if f32:
                    ts.append(T('preds_f32', 'out', exact))
                name = K.launch('kmp_linear_predict', ts, _linear_call(nsp, code, window, p, f32), shift)
                assert name == ('linear_mfma' if mfma else 'linear_valu')


@pytest.mark.parametrize('dtype', [np.uint8, np.uint16], ids=['uint8', 'uint16'])
@pytest.mark.parametrize('case', LINEAR, ids=['x'.join(map(str, c[1])) for c in LINEAR])
def test_linear_predict_mfma(kom, dtype, case):
    nsp, cells, pads = case
    code = CODE[np.dtype(dtype)]
    for p in pads:
        window, w, b, feats = _linear_case(nsp, cells, p, dtype)
        split = OP.linear_bf16x2_split(feats, w, b)  # float64
        n_axis = feats.ndim - 2
        scale = np.tensordot(np.moveaxis(np.abs(feats.astype(np.float64)), n_axis, -1), np.abs(w.astype(np.float64)),
                             axes=([-1], [0]))
        tol = 1e-5 * (np.moveaxis(scale, -1, n_axis) + np.abs(b.astype(np.float64)).reshape(-1, 1))
        lo_int = OC.cast_from_f32((split - tol).astype(np.float32), dtype).astype(np.int64)
        hi_int = OC.cast_from_f32((split + tol).astype(np.float32), dtype).astype(np.int64)

        def far(v):  # the float32 cells: outside the bound (NaN counts as outside)
            return ~(np.abs(v.astype(np.float64) - split) <= tol)

        def off(v):  # the integer cells: outside the casts of the bound's ends (the cast is monotone,
            # and so is the float32 rounding of the ends, which a float32 cell inside them cannot pass)
            return (v.astype(np.int64) < lo_int) | (v.astype(np.int64) > hi_int)

        for f32 in (True, False):
            for shift in K.SHIFTS:
                ts = [T('window', 'in', window), T('weights', 'in', w), T('bias', 'in', b),
                      T('preds', 'out', np.zeros(split.shape, dtype), judge=off)]
                if f32:
                    ts.append(T('preds_f32', 'out', np.zeros(split.shape, np.float32), judge=far))
                keep = []
                name = K.launch('kmp_linear_predict_mfma', ts, _linear_call(nsp, code, window, p, f32), shift, keep=keep)
                assert name == 'linear_bf16x2'
                for got in keep if f32 else ():  # the integer cells are the cast of the launch's own f32 cells
                    assert np.array_equal(K.payload_numpy(got['preds']),
                                          OC.cast_from_f32(K.payload_numpy(got['preds_f32']), dtype))


def test_every_declared_entry_point_was_launched():
    """Runs last: the ledger counts LAUNCHES as guarded, so each of them must have run above."""
    K.assert_declared_were_launched(LAUNCHES)
