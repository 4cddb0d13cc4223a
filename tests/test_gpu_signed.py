"""Signed samples (int8 / int16) through the fused codec and the Python API, against tests/signed_spec.py:
the codec on signed ``x`` is the oracle's codec on ``M(x) = x ^ signbit``, with every sample-domain array
(lowres, highres, predictions) in the signed type.  Each row pins the maps and lowres bit for bit,
the lossless round trip and the kernel family ``kmp_last_launch()`` names."""

import numpy as np
import pytest
import torch

import oracle
from oracle.common import cast_from_f32
import signed_spec as S

pytestmark = pytest.mark.gpu

I8, I16 = np.int8, np.int16
NP2T = {np.dtype(I8): torch.int8, np.dtype(I16): torch.int16}

# (id, shape, dtypes, predictor, padding, family)
ROWS = [
    ('vol-p0', (2, 12, 16, 64, 1), (I16, I8), 'mean', 0, 'wave3d'),
    ('vol-p0-odd', (2, 11, 16, 64, 1), (I16, I8), 'mean', 0, 'wave3d'),
    ('img-p0', (2, 32, 64, 1), (I16, I8), 'mean', 0, 'wave2d'),
    ('img-p0-odd', (2, 31, 64, 1), (I16, I8), 'mean', 0, 'wave2d'),
    ('vol-c3', (1, 8, 16, 32, 3), (I16, I8), 'mean', 0, 'generic'),
    ('vol-w48-p1', (2, 9, 12, 48, 1), (I16, I8), 'mean', 1, 'generic'),
    ('vol-lin-p0', (2, 9, 10, 12, 1), (I16, I8), 'f32', 0, 'generic'),
    ('vol-lin-p1', (2, 8, 9, 7, 1), (I16, I8), 'f32', 1, 'generic'),
    ('img-lin-p0', (3, 33, 20, 1), (I16,), 'f32', 0, 'generic'),
    # the image wave kernel's LinearPredictor arm runs on the mapped nodes like its mean arm
    ('img-lin-p0-wave', (3, 64, 64, 1), (I16, I8), 'f32', 0, 'wave2d'),
]
CASES = [(r[0], dt) for r in ROWS for dt in r[2]]
ROW_BY_ID = {r[0]: r for r in ROWS}
_REF = {}


def _launch_name(family, direction):
    return f'{direction}_generic' if family == 'generic' else f'{family}_{direction}'


def _coders(ns, dtype):
    name = np.dtype(dtype).name
    return getattr(ns, 'encode_values_' + name), getattr(ns, 'decode_values_' + name)


def _weights(p, ndim):
    return S.clamp_weights((2 * p + 2) ** ndim, 19 if ndim == 3 else 5)


def _oracle_fn(kind, p, ndim):
    return S.mean_fn(p, ndim) if kind == 'mean' else S.linear_fn(p, *_weights(p, ndim), ndim)


def _predictor(kom, kind, p, ndim, arith='f32'):
    if kind == 'mean':
        return kom.MeanPredictor(p, ndim)
    return kom.LinearPredictor(*_weights(p, ndim), p, ndim, arith=arith)


def reference(rid, dtype):
    """{'x', 'lowres', 'maps', 'dims'} of a row from the specification, computed once."""
    key = (rid, np.dtype(dtype).name)
    if key not in _REF:
        _, shape, _, kind, p, _ = ROW_BY_ID[rid]
        ndim = len(shape) - 2
        x = S.data(shape, dtype, seed=len(rid))
        fn = _oracle_fn(kind, p, ndim)
        lo, maps, dims = S.encode(x, fn, ndim, p)
        assert np.array_equal(S.decode(lo, maps, dims, fn, ndim, p), x)
        _REF[key] = {'x': x, 'lowres': lo, 'maps': maps, 'dims': dims}
    return _REF[key]


@pytest.mark.parametrize('rid,dtype', CASES, ids=[f'{r}-{np.dtype(d).name}' for r, d in CASES])
def test_bit_exact_and_routed(kom, rid, dtype):
    _, shape, _, kind, p, family = ROW_BY_ID[rid]
    ndim = len(shape) - 2
    ns = kom.volume if ndim == 3 else kom.image
    enc, dec = _coders(ns, dtype)
    ref = reference(rid, dtype)
    x = ref['x']
    pred = _predictor(kom, kind, p, ndim, arith='auto')
    last = lambda: kom._lib.lib.kmp_last_launch().decode()  # noqa: E731
    lo, (maps, dims) = ns.encode(pred, enc, x, padding=p)
    assert last() == _launch_name(family, 'encode')
    assert lo.dtype == x.dtype and np.array_equal(lo, ref['lowres'])
    assert tuple(dims) == ref['dims']
    for k, (a, b) in enumerate(zip(maps, ref['maps'])):
        assert a.dtype == S.unsigned_of(dtype) and np.array_equal(a, b), f'map {k}'
    sl = (slice(None),) + (slice(None, None, 2),) * ndim
    assert np.array_equal(lo, x[sl])
    back = ns.decode(pred, dec, lo, (maps, dims), padding=p)
    assert last() == _launch_name(family, 'decode')
    assert back.dtype == x.dtype and np.array_equal(back, x)


@pytest.mark.parametrize('dtype', [I16, I8], ids=['int16', 'int8'])
def test_same_maps_as_the_unsigned_codec_on_the_shifted_array(kom, dtype):
    """An encode of signed ``x`` and the product's own encode of the unsigned ``x + 2^(W-1)`` give the same
    maps, on the wave kernel and on the generic path."""
    for shape, p in (((2, 12, 16, 64, 1), 0), ((2, 9, 12, 48, 1), 1)):
        x = S.data(shape, dtype, seed=9)
        u = S.M(x)
        V = kom.volume
        enc, _ = _coders(V, dtype)
        enc_u = getattr(V, 'encode_values_' + u.dtype.name)
        lo, (maps, dims) = V.encode(kom.MeanPredictor(p, 3), enc, x, padding=p)
        lo_u, (maps_u, dims_u) = V.encode(kom.MeanPredictor(p, 3), enc_u, u, padding=p)
        assert tuple(dims) == tuple(dims_u) and np.array_equal(S.M(lo), lo_u)
        for a, b in zip(maps, maps_u):
            assert np.array_equal(a, b)


CHUNKED = [('vol-p0', I16), ('vol-p0-odd', I8), ('img-p0', I8), ('img-p0-odd', I16), ('vol-lin-p0', I16),
           ('vol-w48-p1', I16)]


@pytest.mark.parametrize('rid,dtype', CHUNKED, ids=[f'{r}-{np.dtype(d).name}' for r, d in CHUNKED])
def test_chunks_equal_the_whole_array_call(kom, rid, dtype):
    _, shape, _, kind, p, _ = ROW_BY_ID[rid]
    ndim = len(shape) - 2
    ns = kom.volume if ndim == 3 else kom.image
    enc, dec = _coders(ns, dtype)
    ref = reference(rid, dtype)
    pred = _predictor(kom, kind, p, ndim)
    for chunk in (6, 11):
        lo, (maps, dims) = ns.encode_chunks(pred, enc, ref['x'], chunk=chunk, padding=p)
        assert np.array_equal(lo, ref['lowres']) and lo.dtype == ref['x'].dtype and tuple(dims) == ref['dims']
        for a, b in zip(maps, ref['maps']):
            assert np.array_equal(a, b)
        back = ns.decode_chunks(pred, dec, lo, (maps, dims), chunk=chunk, padding=p)
        assert np.array_equal(back, ref['x']) and back.dtype == ref['x'].dtype


@pytest.mark.parametrize('dtype', [I16, I8], ids=['int16', 'int8'])
def test_pyramid_round_trips(kom, dtype):
    x = S.data((1, 17, 24, 32, 1), dtype, seed=3)
    V = kom.volume
    enc, dec = _coders(V, dtype)
    pred = kom.MeanPredictor(0, 3)
    lo, levels = V.encode_pyramid(pred, enc, x, levels=2, padding=0)
    assert lo.dtype == x.dtype and np.array_equal(lo, x[:, ::4, ::4, ::4])
    assert np.array_equal(V.decode_pyramid(pred, dec, lo, levels, padding=0), x)


@pytest.mark.parametrize('dtype', [I16, I8], ids=['int16', 'int8'])
def test_stand_alone_coders(kom, dtype):
    """``(gt - pred) mod 2^W`` on the signed values, numpy and torch, aligned and odd lengths; the decoder
    returns the signed type."""
    U = kom.utils
    enc, dec = _coders(U, dtype)
    for n in (4096, 4097, 5):
        gt, pred = S.uniform((n,), dtype, 1), S.uniform((n,), dtype, 2)
        gt[:5], pred[:5] = S.extremes(dtype), S.extremes(dtype)[::-1]
        want = S.encode_values(pred, gt)
        got = enc(pred, gt)
        assert got.dtype == want.dtype and np.array_equal(got, want)
        back = dec(pred, got)
        assert back.dtype == np.dtype(dtype) and np.array_equal(back, gt)
        tg = enc(torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda())
        assert tg.dtype == {1: torch.uint8, 2: torch.uint16}[np.dtype(dtype).itemsize]
        assert np.array_equal(tg.cpu().numpy(), want)


@pytest.mark.parametrize('dtype', [I16, I8], ids=['int16', 'int8'])
@pytest.mark.parametrize('ndim,shape', [(3, (2, 6, 7, 9, 1)), (3, (1, 5, 6, 7, 2)), (2, (2, 9, 12, 1))])
@pytest.mark.parametrize('p', [0, 1])
def test_predictor_callables_return_signed_maps(kom, dtype, ndim, shape, p):
    """MeanPredictor and LinearPredictor called on a signed padded-lowres window: ``M^-1`` of the
    unsigned predictor's maps of ``M(window)``, in the signed type."""
    window = S.ons(ndim).pad_neighborhood(S.data(shape, dtype, seed=p + ndim), p)
    for kind in ('mean', 'f32'):
        if kind == 'f32' and shape[-1] != 1:
            continue
        got = _predictor(kom, kind, p, ndim)(window)
        want = S.predictions(window, _oracle_fn(kind, p, ndim))
        assert len(got) == len(want)
        for k, (a, b) in enumerate(zip(got, want)):
            assert a.dtype == np.dtype(dtype) and np.array_equal(a, b), f'{kind} map {k}'


def test_linear_cells_cast_in_the_mapped_domain(kom):
    """Constant predictions (zero weights, bias c) on int16: the cell is M^-1(cast_uint16(c)) -- saturating at
    both ends of the mapped range, truncating, NaN to mapped 0."""
    consts = np.array([-0.0, 0.999, -0.5, -1.0, -8e4, 65534.5, 65535.0, 65535.5, 65536.0, 8e4, 2.0 ** 31, 2.0 ** 32,
                       3e38, np.inf, -np.inf, np.nan, 32768.0, 32767.9, 1e-40], np.float32)
    assert consts.size == 19
    pred = kom.LinearPredictor(np.zeros((8, 19), np.float32), consts, 0, 3, arith='f32')
    window = S.data((1, 3, 4, 5, 1), I16, seed=1)
    cells = pred.predict_cells(window)
    assert cells.dtype == np.int16
    want = S.Minv(cast_from_f32(consts, np.uint16))
    assert want[15] == -32768 and want[13] == 32767 and want[14] == -32768 and want[16] == 0
    assert np.array_equal(cells, np.broadcast_to(want.reshape(1, 1, 1, 1, 19, 1), cells.shape))


PLANTS = (1e9, -np.inf, np.nan, np.inf, -1e9, -5.7, 5.7, 40000.0, -40000.0, 2.0 ** 31, -2.0 ** 31, 3e38)


def _plant(flat):
    flat[:len(PLANTS)] = flat.new_tensor(PLANTS) if isinstance(flat, torch.Tensor) else np.array(PLANTS, np.float32)


@pytest.mark.parametrize('ndim,shape,p', [(3, (2, 9, 10, 12, 1), 1), (2, (2, 13, 16, 1), 0)])
def test_callback_path_with_float32_maps(kom, ndim, shape, p):
    """A torch predictions_fn gets real int16 and returns float32 maps: the coder reads them as int32(pred)
    (truncate toward zero, saturate, NaN -> 0; utils.py:28-55) and codes (gt - pred) mod 2^16 of the
    signed values.  Lossless, equal to the oracle's step sequence with the same maps, through the
    with_predictions launches."""
    ns, o = (kom.volume, oracle.volume) if ndim == 3 else (kom.image, oracle.image)
    x = S.data(shape, I16, seed=6)
    seen = []

    def torch_fn(window):
        assert isinstance(window, torch.Tensor) and window.dtype == torch.int16 and window.is_cuda
        seen.append(window.cpu().numpy())
        maps = [m.to(torch.float32) + 0.25 for m in kom.MeanPredictor(p, ndim)(window)]
        for m in maps:
            _plant(m.view(-1))
        return tuple(maps)

    def numpy_fn(window):
        maps = [m.astype(np.float32) + np.float32(0.25) for m in S.predictions(window, S.mean_fn(p, ndim))]
        for m in maps:
            _plant(m.reshape(-1))
        return tuple(maps)

    def enc_ref(pred, gt):
        return S.encode_values(cast_from_f32(pred, np.int32), gt)

    def dec_ref(pred, e):
        return S.decode_values(cast_from_f32(pred, np.int32), e, np.int16)

    want_lo, (want_maps, want_dims) = o.encode(numpy_fn, enc_ref, x, padding=p)
    assert np.array_equal(o.decode(numpy_fn, dec_ref, want_lo, (want_maps, want_dims), padding=p), x)
    xt = torch.from_numpy(x).cuda()
    lo, (maps, dims) = ns.encode(torch_fn, ns.encode_values_int16, xt, padding=p)
    assert kom._lib.lib.kmp_last_launch().decode() == 'encode_with_predictions'
    assert np.array_equal(seen[0], o.pad_neighborhood(o.lowres_from_highres(o.pad_highres(x)[0]), p))
    assert lo.dtype == torch.int16 and np.array_equal(lo.cpu().numpy(), want_lo) and tuple(dims) == tuple(want_dims)
    for k, (a, b) in enumerate(zip(maps, want_maps)):
        assert a.dtype == torch.uint16 and np.array_equal(a.cpu().numpy(), b), f'map {k}'
    back = ns.decode(torch_fn, ns.decode_values_int16, lo, (maps, dims), padding=p)
    assert kom._lib.lib.kmp_last_launch().decode() == 'decode_with_predictions'
    assert back.dtype == torch.int16 and np.array_equal(back.cpu().numpy(), x)


def test_callback_path_with_numpy_callbacks(kom):
    """Opaque numpy callbacks (no built-in coder recognised): the reference's step sequence on signed
    arrays, every primitive moving int16 as it is."""
    x = S.data((2, 9, 10, 11, 1), I16, seed=8)
    host = lambda t: t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)  # noqa: E731
    fn = lambda w: S.predictions(host(w), S.mean_fn(0, 3))  # noqa: E731
    enc = lambda pr, gt: S.encode_values(host(pr), host(gt))  # noqa: E731
    dec = lambda pr, e: S.decode_values(host(pr), host(e), np.int16)  # noqa: E731
    lo, (maps, dims) = kom.volume.encode(fn, enc, x, padding=0)
    want_lo, want_maps, want_dims = S.encode(x, S.mean_fn(0, 3), 3, 0)
    assert np.array_equal(lo, want_lo) and tuple(dims) == want_dims
    for a, b in zip(maps, want_maps):
        assert np.array_equal(a, b)
    assert np.array_equal(kom.volume.decode(fn, dec, lo, (maps, dims), padding=0), x)


def test_fit_on_signed_data_beats_the_mean(kom):
    """LinearPredictor.fit on the zero-crossing int16 field: fitted in the mapped domain, its mean
    |residual| is no larger than MeanPredictor's on that field."""
    x = S.zero_crossing((1, 32, 32, 32, 1), I16, seed=0)
    V = kom.volume
    m_signed = kom.predictors.linear_moments(x, 0, 3)
    assert np.array_equal(m_signed, kom.predictors.linear_moments(S.M(x), 0, 3))
    lin = kom.LinearPredictor.fit(x, padding=0, ndim=3)
    assert lin.arith_for(torch.int16) == 'f32'

    def mean_abs(pred):
        lo, (maps, dims) = V.encode(pred, V.encode_values_int16, x, padding=0)
        assert np.array_equal(V.decode(pred, V.decode_values_int16, lo, (maps, dims), padding=0), x)
        return float(np.mean(np.concatenate([np.abs(m.view(np.int16).astype(np.int64)).reshape(-1) for m in maps])))

    a, b = mean_abs(lin), mean_abs(kom.MeanPredictor(0, 3))
    print(f'mean |residual|: fitted LinearPredictor {a:.3f}, MeanPredictor {b:.3f}')
    assert a <= b


def test_errors(kom):
    from kompressor_amd import _nd, _lib
    V = kom.volume
    x = S.data((1, 8, 8, 16, 1), I16, seed=1)
    lin = kom.LinearPredictor(*_weights(1, 3), 1, 3, arith='bf16x2')
    with pytest.raises(ValueError, match='bf16x2'):
        V.encode(lin, V.encode_values_int16, x, padding=1)
    auto = kom.LinearPredictor(*_weights(1, 3), 1, 3)
    assert auto.arith_for(torch.int16) == 'f32' and auto.arith_for(torch.int8) == 'f32'
    assert auto.arith_for(torch.uint16) == 'bf16x2'
    # the uint8 coder is not int16's: no fused route (the call runs the reference's steps instead)
    assert _nd.fused_plan(kom.MeanPredictor(0, 3), V.encode_values_uint8, 0, torch.int16, 3, _lib.ENCODE) is None
    assert _nd.fused_plan(kom.MeanPredictor(0, 3), V.encode_values_int16, 0, torch.int16, 3, _lib.ENCODE) is not None
    # the matrix-core kind with a signed dtype is refused by the C front door, with a message
    xt = torch.from_numpy(x).cuda()
    lo, maps, dims = _nd._alloc_encoded(xt, _lib.CODER_U16, 3)

    class Mfma:
        def _kmp_predictor(self, dtype):
            w, b = lin._device_params()
            return _lib.Predictor(_lib.PRED_LINEAR_MFMA, 1, w.data_ptr(), b.data_ptr())

    with pytest.raises(_lib.KompressorHipError, match='matrix-core'):
        _nd.fused_encode_into(xt, Mfma(), _lib.CODER_U16, lo, maps, 3)


@pytest.mark.parametrize('name,ndim', [('signed_vol_i16', 3), ('signed_img_i8', 2)])
@pytest.mark.parametrize('padding', [0, 1])
def test_golden_fixtures(kom, name, ndim, padding):
    """The committed vectors (tests/golden/make_golden_signed.py): encode gives them, decode inverts them."""
    from conftest import golden_maps, load_golden
    g = load_golden(f'{name}_p{padding}')
    x = g['highres']
    ns = kom.volume if ndim == 3 else kom.image
    enc, dec = _coders(ns, x.dtype)
    pred = kom.MeanPredictor(padding, ndim)
    lo, (maps, dims) = ns.encode(pred, enc, x, padding=padding)
    assert lo.dtype == x.dtype and np.array_equal(lo, g['lowres']) and tuple(dims) == tuple(g['dims'])
    for a, b in zip(maps, golden_maps(g, ndim)):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    back = ns.decode(pred, dec, g['lowres'], (golden_maps(g, ndim), tuple(int(d) for d in g['dims'])), padding=padding)
    assert np.array_equal(back, x)
