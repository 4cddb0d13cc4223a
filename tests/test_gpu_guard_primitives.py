"""Guard bands, exact ownership and off-alignment pointers for the geometry primitives and the
coders of the C-ABI (kmp_primitives.hip, kmp_tiles.hip, kmp_categorical.hip; the predictor primitives
of kmp_maps_from_predictions.hip and kmp_mean_predict.hip: test_gpu_guard_callback.py), called directly through
``kompressor_amd._lib.lib`` with pointers into sentinel-filled arenas (guard_capi.py, guard_spec.py).

Per launch, twice (0xA5 / 0x5A arenas): guards, shift bytes and inputs unchanged; output elements the
launch does not own still the sentinel; owned elements bit-equal to the numpy oracle; the two runs
identical.  Every case runs with all pointers aligned, with every tensor moved by one element of its
dtype, and with only the outputs moved; the row kernels (C == 1) and the element kernels
(KMP_DISABLE_ROWS=1, and C == 3) both run.

Row lengths: with V = 16 / sizeof(T) samples per 16-byte chunk, w in {3, 2V-1, 2V, 2V+1, 2V+2, 4V+1}
(one partial chunk; a chunk boundary on either side of the 2V-wide parity split, even and odd so
``dims`` is 1 and 0; a second chunk).  The other axes alternate between (5, 6) and (6, 5) (images: 7
and 8 rows), so both parities of every axis occur per dtype.
"""

import numpy as np
import pytest

from oracle import common as OC
import guard_spec as G
import guard_capi as K
from guard_capi import T, CODE, DTYPES, DT_IDS, widths, shapes, ons, form  # noqa: F401  (form: a fixture)

pytestmark = pytest.mark.gpu

# the entry points this module puts under guard (read by the ledger, test_guard_ledger.py)
LAUNCHES = ('kmp_lowres_from_highres', 'kmp_maps_from_highres', 'kmp_targets_from_highres',
            'kmp_highres_from_lowres_and_maps', 'kmp_features_from_lowres', 'kmp_pad', 'kmp_copy_box', 'kmp_tiles',
            'kmp_code', 'kmp_categorical')

PADS = [((0, 0, 0), (1, 1, 1)), ((2, 1, 3), (2, 0, 5)), ((1, 2, 17), (0, 3, 9)), ((0, -1, -2), (1, 0, -3))]


def _maps(prefix, arrays, role):
    return [T(f'{prefix}{k}', role, a) for k, a in enumerate(arrays)]


# ---------------------------------------------------------------------------------------------
# deinterleave / interleave / targets
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize('nsp', [3, 2])
@pytest.mark.parametrize('dtype', DTYPES, ids=DT_IDS)
def test_lowres_and_maps_from_highres(kom, form, dtype, nsp):
    code = CODE[np.dtype(dtype)]
    for shape in shapes(dtype, nsp):
        x = K.rand(shape, dtype, shape[-2])
        sp, C = shape[1:1 + nsp], shape[-1]
        lo, maps = ons(nsp).lowres_from_highres(x), ons(nsp).maps_from_highres(x)
        for shift in K.SHIFTS:
            name = K.launch('kmp_lowres_from_highres', [T('highres', 'in', x), T('lowres', 'out', lo)],
                            lambda fn, p: fn(nsp, code, p['highres'], shape[0], K.i64x3(sp), C, p['lowres'], None),
                            shift)
            assert name == 'lowres_from_highres'
            outs = _maps('map', maps, 'out')
            name = K.launch('kmp_maps_from_highres', [T('highres', 'in', x)] + outs,
                            lambda fn, p: fn(nsp, code, p['highres'], shape[0], K.i64x3(sp), C,
                                             K.ptr_array([p[t.name] for t in outs]), None), shift)
            assert name == 'maps_from_highres'


@pytest.mark.parametrize('nsp', [3, 2])
@pytest.mark.parametrize('dtype', DTYPES, ids=DT_IDS)
def test_highres_from_lowres_and_maps(kom, form, dtype, nsp):
    """The merge on the odd-extent siblings ``s | 1`` of the shapes (an interleaved grid is odd)."""
    code = CODE[np.dtype(dtype)]
    for shape in shapes(dtype, nsp):
        odd = (shape[0], *[s | 1 for s in shape[1:1 + nsp]], shape[-1])
        x = K.rand(odd, dtype, shape[-2] + 1)
        lo, maps = ons(nsp).lowres_from_highres(x), ons(nsp).maps_from_highres(x)
        assert np.array_equal(ons(nsp).highres_from_lowres_and_maps(lo, maps), x)
        ins = _maps('map', maps, 'in')
        for shift in K.SHIFTS:
            name = K.launch('kmp_highres_from_lowres_and_maps', [T('lowres', 'in', lo)] + ins + [T('highres', 'out', x)],
                            lambda fn, p: fn(nsp, code, p['lowres'], K.ptr_array([p[t.name] for t in ins]), odd[0],
                                             K.i64x3(lo.shape[1:1 + nsp]), odd[-1], p['highres'], None), shift)
            assert name == 'highres_from_lowres_and_maps'


@pytest.mark.parametrize('nsp', [3, 2])
@pytest.mark.parametrize('dtype', DTYPES, ids=DT_IDS)
def test_targets_from_highres(kom, form, dtype, nsp):
    """An even extent n has (n - 1) / 2 cells, those of its first n - 1 samples: the oracle (whose
    slices need odd extents) runs on that crop, the kernel on the whole array with its strides."""
    code = CODE[np.dtype(dtype)]
    for shape in shapes(dtype, nsp):
        x = K.rand(shape, dtype, shape[-2] + 2)
        sp, C = shape[1:1 + nsp], shape[-1]
        crop = x[(slice(None), *[slice(0, s - 1 + s % 2) for s in sp])]
        want = ons(nsp).targets_from_highres(crop)
        assert want.shape == (shape[0], *[(s - 1) // 2 for s in sp], 19 if nsp == 3 else 5, C)
        for shift in K.SHIFTS:
            name = K.launch('kmp_targets_from_highres', [T('highres', 'in', x), T('targets', 'out', want)],
                            lambda fn, p: fn(nsp, code, p['highres'], shape[0], K.i64x3(sp), C, p['targets'], None),
                            shift)
            assert name == 'targets_from_highres'


# ---------------------------------------------------------------------------------------------
# features
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize('p', [0, 1, 2])
@pytest.mark.parametrize('nsp', [3, 2])
@pytest.mark.parametrize('dtype', DTYPES, ids=DT_IDS)
def test_features_from_lowres(kom, form, dtype, nsp, p):
    """The window is the shape padded by p (so every shape has cells at every p).  The 16-byte vector
    kernel serves 8 / 16-bit C == 1 windows at p <= 1 when ``out`` is 16-byte aligned; besides the three
    common shifts, only the input moved (the vector kernel must still be exact) and -- the 'out' mode
    -- only the output moved (the fallback's turn)."""
    code = CODE[np.dtype(dtype)]
    item = np.dtype(dtype).itemsize
    for shape in shapes(dtype, nsp):
        lowres = ons(nsp).pad_neighborhood(K.rand(shape, dtype, shape[-2] + p), p)
        want = ons(nsp).features_from_lowres(lowres, p)
        S, C = lowres.shape[1:1 + nsp], shape[-1]
        for shift in K.SHIFTS + ({'lowres': item},):
            name = K.launch('kmp_features_from_lowres', [T('lowres', 'in', lowres), T('features', 'out', want)],
                            lambda fn, q: fn(nsp, code, q['lowres'], shape[0], K.i64x3(S), C, p, q['features'], None),
                            shift)
            assert name == 'features_from_lowres'


# ---------------------------------------------------------------------------------------------
# pad / crop
# ---------------------------------------------------------------------------------------------

def _np_pad(x, lo, hi, mode):
    pos = [(max(a, 0), max(b, 0)) for a, b in zip(lo, hi)]  # numpy pads first, then the negative pads crop
    ref = np.pad(x, [(0, 0), *pos, (0, 0)], mode='symmetric' if mode == 0 else 'reflect')
    sl = [slice(None)] + [slice(-min(a, 0), ref.shape[i + 1] + min(b, 0)) for i, (a, b) in enumerate(zip(lo, hi))]
    return np.ascontiguousarray(ref[tuple(sl)])


@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('nsp', [3, 2])
@pytest.mark.parametrize('dtype', DTYPES, ids=DT_IDS)
def test_pad(kom, form, dtype, nsp, mode):
    """jnp.pad / trim: the four pad sets of test_rows_pad (images: their y, x entries), wherever numpy
    defines the result (a positive output extent; 'reflect' pads below the axis length)."""
    code = CODE[np.dtype(dtype)]
    ran = 0
    for shape in shapes(dtype, nsp):
        x = K.rand(shape, dtype, shape[-2] + 3)
        sp, C = shape[1:1 + nsp], shape[-1]
        for lo, hi in PADS:
            lo, hi = lo[3 - nsp:], hi[3 - nsp:]
            if any(s + a + b <= 0 for s, a, b in zip(sp, lo, hi)):
                continue
            if mode == 1 and any(max(a, b) >= s for s, a, b in zip(sp, lo, hi)):
                continue
            want = _np_pad(x, lo, hi, mode)
            for shift in K.SHIFTS:
                name = K.launch('kmp_pad', [T('in', 'in', x), T('out', 'out', want)],
                                lambda fn, p: fn(nsp, code, p['in'], shape[0], K.i64x3(sp), C, K.i64x3(lo), K.i64x3(hi),
                                                 mode, p['out'], None), shift)
                assert name == 'pad'
                ran += 1
    assert ran >= 3 * (len(shapes(dtype, nsp)) + 8)  # every shape takes the first set; most take more


# ---------------------------------------------------------------------------------------------
# box copy
# ---------------------------------------------------------------------------------------------

def _convert(a, dtype):
    if np.dtype(dtype) == a.dtype:
        return a
    if a.dtype == np.float32:
        return OC.cast_from_f32(a, dtype)  # the XLA truncating cast
    return a.astype(dtype)                # integer narrowing wraps


@pytest.mark.parametrize('pair', [(np.uint8, np.uint8), (np.uint16, np.uint16), (np.int32, np.int32),
                                  (np.float32, np.float32), (np.uint32, np.uint32), (np.int32, np.uint8),
                                  (np.float32, np.uint16)],
                         ids=lambda p: f'{np.dtype(p[0]).name}-{np.dtype(p[1]).name}')
def test_copy_box(kom, form, pair):
    """x extent w - 2 at in / out x offsets 0, 1 and 4: the launch owns the box; the rest of ``dst``
    keeps the sentinel.  Converting pairs take the element kernel."""
    din, dout = pair
    for i, w in enumerate(widths(dout)):
        for nsp, C in ((3, 1), (2, 1)) + (((3, 3),) if i == 0 else ()):
            ex = max(w - 2, 1)
            if nsp == 3:
                src_sp, dst_sp = ((7, 6, ex + 4), (9, 8, ex + 7)) if i % 2 == 0 else ((6, 7, ex + 4), (8, 9, ex + 7))
                ext, ioff, ooff = (5, 4, ex), (1, 2), (3, 1)
            else:
                src_sp, dst_sp = ((7, ex + 4), (9, ex + 7)) if i % 2 == 0 else ((8, ex + 4), (8, ex + 7))
                ext, ioff, ooff = (5, ex), (2,), (1,)
            src = K.rand((2, *src_sp, C), din, w)
            for xi in (0, 1, 4):
                for xo in (0, 1, 4):
                    io, oo = (*ioff, xi), (*ooff, xo)
                    want = np.zeros((2, *dst_sp, C), dout)
                    box = tuple(slice(o, o + e) for o, e in zip(oo, ext))
                    want[(slice(None), *box)] = _convert(src[(slice(None), *[slice(o, o + e) for o, e in zip(io, ext)])],
                                                         dout)
                    mask = G.copy_box_mask(want.shape, oo, ext, nsp)
                    for shift in K.SHIFTS:
                        name = K.launch('kmp_copy_box', [T('src', 'in', src), T('dst', 'out', want, mask=mask)],
                                        lambda fn, p: fn(nsp, CODE[np.dtype(din)], p['src'], K.i64x3(src_sp),
                                                         K.i64x3(io), CODE[np.dtype(dout)], p['dst'], K.i64x3(dst_sp),
                                                         K.i64x3(oo), 2, C, K.i64x3(ext), None), shift)
                        assert name == 'copy_box'


# ---------------------------------------------------------------------------------------------
# tiles
# ---------------------------------------------------------------------------------------------

def _tiles(x, tile):
    """[D, H, W, C] -> [n, Tz, Ty, Tx, C] in z-major tile order, by reshape and transpose."""
    nsp = len(tile)
    counts = [s // t for s, t in zip(x.shape[:nsp], tile)]
    split = x.reshape(*[v for c, t in zip(counts, tile) for v in (c, t)], x.shape[-1])
    order = [2 * a for a in range(nsp)] + [2 * a + 1 for a in range(nsp)] + [2 * nsp]
    return np.ascontiguousarray(split.transpose(order).reshape(-1, *tile, x.shape[-1]))


@pytest.mark.parametrize('C', [1, 3])
@pytest.mark.parametrize('dtype', DTYPES, ids=DT_IDS)
def test_tiles(kom, dtype, C):
    code = CODE[np.dtype(dtype)]
    for shape, tile in (((8, 8, 16), (4, 4, 8)), ((8, 32), (4, 16))):
        nsp = len(tile)
        whole = K.rand((*shape, C), dtype, 7 + nsp)
        batch = _tiles(whole, tile)
        assert batch.shape[0] == 8 if nsp == 3 else batch.shape[0] == 4
        assert np.array_equal(batch[1, ..., 0], whole[(*[slice(0, t) for t in tile[:-1]],
                                                      slice(tile[-1], 2 * tile[-1]), 0)])
        for shift in K.SHIFTS:
            for direction, src, dst in ((0, whole, batch), (1, batch, whole)):
                K.launch('kmp_tiles', [T('src', 'in', src), T('dst', 'out', dst)],
                         lambda fn, p: fn(nsp, code, direction, p['src'], K.i64x3(shape), C, K.i64x3(tile), p['dst'],
                                          None), shift)


# ---------------------------------------------------------------------------------------------
# residual coders
# ---------------------------------------------------------------------------------------------

CODERS = {  # coder id: (name, output dtype)
    0: ('raw', np.int32), 1: ('uint8', np.uint8), 2: ('uint16', np.uint16), 3: ('uint32', np.uint32)}
# (pred dtype, sample dtype): same-width integer operands reach the 16-byte vector kernel when all three
# pointers are 16-byte aligned and n % V == 0; a mixed-width and a float32-prediction pair never do
CODE_PAIRS = {
    0: [(np.int32, np.int32), (np.uint8, np.uint8), (np.float32, np.uint16)],
    1: [(np.uint8, np.uint8), (np.uint16, np.uint8), (np.float32, np.uint8)],
    2: [(np.uint16, np.uint16), (np.uint8, np.uint16), (np.float32, np.uint16)],
    3: [(np.uint32, np.uint32), (np.uint16, np.uint32)],
}


@pytest.mark.parametrize('direction', [0, 1], ids=['encode', 'decode'])
@pytest.mark.parametrize('coder', [0, 1, 2, 3], ids=[CODERS[c][0] for c in range(4)])
def test_code(kom, coder, direction):
    """n around the vector length V = 16 / sizeof(x): besides the three common shifts, only ``pred``
    and only ``x`` moved, so each term of the vector kernel's alignment test is the one that fails."""
    cname, odt = CODERS[coder]
    fn_np = getattr(OC, ('encode' if direction == 0 else 'decode') + '_values_' + cname)
    for pdt, sdt in CODE_PAIRS[coder]:
        xdt = sdt if direction == 0 else odt  # x = gt for ENCODE, the coded residual for DECODE
        V = 16 // np.dtype(xdt).itemsize
        for n in (1, V - 1, V, V + 1, 5 * V, 5 * V + 3):
            pred, x = K.rand((n,), pdt, n), K.rand((n,), xdt, n + 1)
            want = fn_np(pred, x)
            assert want.dtype == np.dtype(odt) and want.shape == (n,)
            shifts = K.SHIFTS + ({'pred': np.dtype(pdt).itemsize}, {'x': np.dtype(xdt).itemsize})
            for shift in shifts:
                name = K.launch('kmp_code', [T('pred', 'in', pred), T('x', 'in', x), T('out', 'out', want)],
                                lambda fn, p: fn(direction, coder, CODE[np.dtype(pdt)], p['pred'], CODE[np.dtype(xdt)],
                                                 p['x'], n, p['out'], None), shift)
                assert name == 'code'


@pytest.mark.parametrize('direction', [0, 1], ids=['encode', 'decode'])
@pytest.mark.parametrize('L,dtype', [(4, np.uint8), (8, np.uint16), (65, np.uint8), (256, np.uint8), (260, np.uint16),
                                     (5, np.int32)], ids=lambda v: str(v) if isinstance(v, int) else np.dtype(v).name)
def test_categorical(kom, direction, L, dtype):
    """Logits at shift 0 and at +4 bytes (one float: rows of L floats then start off every 16-byte
    boundary); values and ranks at the three common shifts."""
    fn_np = OC.encode_categorical if direction == 0 else OC.decode_categorical
    for n in (1, 63, 64, 65, 513):
        rng = np.random.default_rng(1000 * L + n)
        logits = rng.standard_normal((n, L)).astype(np.float32)
        x = rng.integers(0, L, size=(n,)).astype(dtype)
        want = fn_np(logits, x)
        assert want.dtype == np.dtype(dtype) and want.shape == (n,)
        item = np.dtype(dtype).itemsize
        for lshift in (0, 4):
            for mode in K.SHIFTS:
                shift = {'logits': lshift, 'x': item if mode == 'all' else 0, 'out': item if mode != 'none' else 0}
                name = K.launch('kmp_categorical', [T('logits', 'in', logits), T('x', 'in', x), T('out', 'out', want)],
                                lambda fn, p: fn(direction, p['logits'], n, L, CODE[np.dtype(dtype)], p['x'], p['out'],
                                                 None), shift)
                assert name


def test_every_declared_entry_point_was_launched():
    """Runs last: the ledger counts LAUNCHES as guarded, so each of them must have run above."""
    K.assert_declared_were_launched(LAUNCHES)
