"""Near-lossless coding on the device, against tests/near_spec.py bit for bit: kmp_code with the near
codes, one level through every route (the fused generic family, map by map, an opaque torch
predictions_fn with sample-dtype and float32 maps), box regions, the chunked drivers, the closed-loop
pyramid, and determinism."""

import numpy as np
import pytest
import torch

import guard_capi as K
import guard_spec as G
import near_spec as NS

pytestmark = pytest.mark.gpu

NP2T = {np.dtype(np.uint8): torch.uint8, np.dtype(np.uint16): torch.uint16, np.dtype(np.int8): torch.int8,
        np.dtype(np.int16): torch.int16}
DT_IDS = [np.dtype(d).name for d in NS.DTYPES]
PREDICTORS = [('mean', 0), ('mean', 1), ('mean', 2), ('linear', 0), ('linear', 1)]
P_IDS = [f'{k}-p{p}' for k, p in PREDICTORS]


def deltas(dtype):
    return (1, 3, NS.max_delta(dtype))


def shapes(dtype, ndim):
    ws = K.widths(dtype)
    if ndim == 3:
        return [(2, 5, 6, w, 1) if i % 2 == 0 else (2, 6, 5, w, 1) for i, w in enumerate(ws)] + [(1, 5, 6, 7, 3)]
    return [(3, 7, w, 1) for w in ws] + [(2, 7, 9, 3)]


def predictor(kom, kind, p, ndim):
    if kind == 'mean':
        return kom.MeanPredictor(p, ndim)
    w, b = NS.linear_weights(p, ndim)
    return kom.LinearPredictor(w, b, p, ndim, arith='f32')


def spec_fn(kind, p, ndim, dtype):
    if kind == 'mean':
        return NS.mean_fn(p, ndim, dtype)
    w, b = NS.linear_weights(p, ndim)
    return NS.linear_fn(p, w, b, ndim, dtype)


def last(kom):
    return kom._lib.lib.kmp_last_launch().decode()


def host(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


# ---------------------------------------------------------------------------------------------
# kmp_code
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', NS.DTYPES, ids=DT_IDS)
def test_code_tables(kom, dtype):
    """Every (P, x) pair of the 8-bit types, the boundary predictions against every x of the 16-bit
    ones, both directions."""
    for delta in (NS.U8_DELTAS if NS.width(dtype) == 8 else NS.U16_DELTAS):
        pred, x = NS.pair_table(dtype, delta)
        enc_fn, dec_fn = kom.near.coders(dtype, delta)
        want = NS.encode_values(pred, x, delta)
        got = enc_fn(pred, x)
        assert last(kom) == 'code'
        assert got.dtype == want.dtype and np.array_equal(got, want), f'delta {delta}'
        back = dec_fn(pred, got)
        assert back.dtype == np.dtype(dtype)
        assert np.array_equal(back, NS.decode_values(pred, want, delta, dtype)), f'delta {delta}'
        assert np.abs(back.astype(np.int64) - x.astype(np.int64)).max() <= delta
        # a decode of residuals no encoder of this prediction made: still the rule, no wrap
        other = np.roll(want, 12345)
        assert np.array_equal(dec_fn(pred, other), NS.decode_values(pred, other, delta, dtype))


@pytest.mark.parametrize('dtype', NS.DTYPES, ids=DT_IDS)
def test_code_float32_predictions(kom, dtype):
    n = 4099
    pred = NS.f32_predictions(n, dtype)
    x = NS.noise((1, n, 1), dtype, 9).reshape(-1)
    for delta in deltas(dtype):
        enc_fn, dec_fn = kom.near.coders(dtype, delta)
        want = NS.encode_values(pred, x, delta)
        got = enc_fn(torch.from_numpy(pred).cuda(), torch.from_numpy(x).cuda())
        assert got.dtype == NP2T[want.dtype] and np.array_equal(host(got), want)
        back = dec_fn(torch.from_numpy(pred).cuda(), got)
        assert back.dtype == NP2T[np.dtype(dtype)]
        assert np.array_equal(host(back), NS.decode_values(pred, want, delta, dtype))
        assert np.abs(host(back).astype(np.int64) - x.astype(np.int64)).max() <= delta


def test_code_argument_checks(kom):
    from kompressor_amd import _lib
    lib = _lib.lib
    a = torch.zeros(16, dtype=torch.uint8, device='cuda')
    w = torch.zeros(16, dtype=torch.int32, device='cuda')
    call = lambda coder, pdt, xdt, t=a: lib.kmp_code(0, coder, pdt, t.data_ptr(), xdt, t.data_ptr(), 4, t.data_ptr(),  # noqa: E731
                                                     None)
    near8, near16 = _lib.CODER_NEAR_U8, _lib.CODER_NEAR_U16
    assert call(_lib.coder_near(near8, 1), _lib.U8, _lib.U8) == _lib.KMP_OK
    assert call(_lib.CODER_U8 | (1 << 8), _lib.U8, _lib.U8) == _lib.KMP_ERR_ARG        # lossless code, high bits
    assert call(near8, _lib.U8, _lib.U8) == _lib.KMP_ERR_ARG                            # delta 0
    assert call(_lib.coder_near(near8, 128), _lib.U8, _lib.U8) == _lib.KMP_ERR_ARG      # delta too large
    assert call(_lib.coder_near(near16, 32768), _lib.U16, _lib.U16) == _lib.KMP_ERR_ARG
    assert call(_lib.coder_near(near16, 1), _lib.U8, _lib.U8) == _lib.KMP_ERR_ARG       # width mismatch
    assert call(_lib.coder_near(near8, 1), _lib.I16, _lib.I16) == _lib.KMP_ERR_ARG
    assert call(_lib.coder_near(near8, 1), _lib.U16, _lib.U8) == _lib.KMP_ERR_ARG       # predictions of another dtype
    for wide in (_lib.I32, _lib.U32, _lib.F32):
        assert call(_lib.coder_near(near16, 1), wide, wide, w) == _lib.KMP_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert not a.any() and not w.any()


# ---------------------------------------------------------------------------------------------
# one level
# ---------------------------------------------------------------------------------------------

_REF = {}


def reference(dtype, shape, kind, p, delta):
    """The spec's encode and decode of one case, computed once."""
    key = (np.dtype(dtype).name, shape, kind, p, delta)
    if key not in _REF:
        ndim = len(shape) - 2
        x = NS.noise(shape, dtype, seed=sum(shape) + p)
        fn = spec_fn(kind, p, ndim, dtype)
        lo, maps, dims = NS.encode_level(x, fn, ndim, p, delta)
        rec = NS.decode_level(lo, maps, dims, fn, ndim, p, delta)
        assert np.abs(rec.astype(np.int64) - x.astype(np.int64)).max() <= delta
        _REF[key] = {'x': x, 'lowres': lo, 'maps': maps, 'dims': dims, 'rec': rec}
    return _REF[key]


def check_encoded(got, ref, what):
    lo, (maps, dims) = got
    assert tuple(dims) == ref['dims'], what
    assert host(lo).dtype == ref['lowres'].dtype and np.array_equal(host(lo), ref['lowres']), f'{what}: lowres'
    for k, (a, b) in enumerate(zip(maps, ref['maps'])):
        assert host(a).dtype == b.dtype and np.array_equal(host(a), b), f'{what}: map {k}'


@pytest.mark.parametrize('kind,p', PREDICTORS, ids=P_IDS)
@pytest.mark.parametrize('ndim', [3, 2])
@pytest.mark.parametrize('dtype', NS.DTYPES, ids=DT_IDS)
def test_one_level_every_route(kom, monkeypatch, dtype, ndim, kind, p):
    """Fused (the generic family), map by map (KOMPRESSOR_AMD_FUSED=0) and an opaque torch
    predictions_fn with sample-dtype and float32 maps: the spec's bits on every route."""
    ns = kom.volume if ndim == 3 else kom.image
    pred = predictor(kom, kind, p, ndim)
    f32 = lambda w: tuple(torch.from_numpy(host(m).astype(np.float32)).cuda() for m in pred(w))  # noqa: E731
    routes = {'fused': (pred, '1', ('encode_generic', 'decode_generic')),
              'maps': (pred, '0', ('code', None)),
              'callback': (lambda w: pred(w), '1', ('encode_with_predictions', 'decode_with_predictions')),
              'callback-f32': (f32, '1', ('encode_with_predictions', 'decode_with_predictions'))}
    for shape in shapes(dtype, ndim):
        for delta in deltas(dtype):
            ref = reference(dtype, shape, kind, p, delta)
            enc_fn, dec_fn = kom.near.coders(dtype, delta)
            xt = torch.from_numpy(ref['x']).cuda()
            for route, (fn, fused, names) in routes.items():
                what = f'{route} {shape} delta {delta}'
                monkeypatch.setenv('KOMPRESSOR_AMD_FUSED', fused)
                got = ns.encode(fn, enc_fn, xt, padding=p)
                if names[0] != 'code':
                    assert last(kom) == names[0], what
                check_encoded(got, ref, what)
                back = ns.decode(fn, dec_fn, got[0], got[1], padding=p)
                if names[1]:
                    assert last(kom) == names[1], what
                assert back.dtype == NP2T[np.dtype(dtype)] and np.array_equal(host(back), ref['rec']), what


@pytest.mark.parametrize('dtype', [np.uint16, np.int8], ids=['uint16', 'int8'])
@pytest.mark.parametrize('shape,kind,p', [((2, 6, 5, 17, 1), 'mean', 1), ((1, 5, 6, 7, 3), 'linear', 0),
                                          ((3, 7, 33, 1), 'linear', 1), ((2, 7, 9, 3), 'mean', 0)],
                         ids=['vol-row', 'vol-c3', 'img-fused-linear', 'img-c3'])
def test_box_region_decode(kom, dtype, shape, kind, p):
    """A box kmp_region decode writes the same box of the whole decode, and nothing else."""
    from kompressor_amd import _nd
    ndim = len(shape) - 2
    delta = 3
    ref = reference(dtype, shape, kind, p, delta)
    pred = predictor(kom, kind, p, ndim)
    coder = kom.near.coder_id(dtype, delta)
    lo = torch.from_numpy(ref['lowres']).cuda()
    maps = [torch.from_numpy(m).cuda() for m in ref['maps']]
    E = ref['lowres'].shape[1:1 + ndim]
    region = [(1, e) if a % 2 == 0 else (0, max(e - 1, 1)) for a, e in enumerate(E)]
    td = NP2T[np.dtype(dtype)]
    sentinel = 0x5A
    out = torch.empty(ref['x'].shape, dtype=td, device='cuda')
    out.view(torch.uint8).fill_(sentinel)
    before = host(out).copy()
    _nd.fused_decode_into(lo, maps, ref['dims'], pred, coder, out, ndim, region=region)
    assert last(kom) == 'decode_generic'
    mask = G.decode_masks(ref['x'].shape, ref['lowres'].shape, region, ndim)['highres']
    got = host(out)
    assert mask.any() and not mask.all()
    assert np.array_equal(got[mask], ref['rec'][mask])
    assert np.array_equal(got[~mask], before[~mask])
    # and the encode of the same box
    lo2, maps2, _ = _nd._alloc_encoded(torch.from_numpy(ref['x']).cuda(), coder, ndim)
    for t in (lo2, *maps2):
        t.view(torch.uint8).fill_(sentinel)
    _nd.fused_encode_into(torch.from_numpy(ref['x']).cuda(), pred, coder, lo2, maps2, ndim, region=region)
    assert last(kom) == 'encode_generic'
    masks = G.encode_masks(ref['lowres'].shape, [m.shape for m in ref['maps']], region, ndim)
    for name, t, want in [('lowres', lo2, ref['lowres'])] + [(f'map{k}', t, w) for k, (t, w) in
                                                            enumerate(zip(maps2, ref['maps']))]:
        g, m = host(t), masks[name]
        assert np.array_equal(g[m], want[m]), name
        assert (g.view(np.uint8).reshape(*g.shape, -1)[~m] == sentinel).all(), name


@pytest.mark.parametrize('dtype', [np.uint8, np.int16], ids=['uint8', 'int16'])
@pytest.mark.parametrize('shape,kind,p,chunk', [((2, 9, 10, 13, 1), 'mean', 1, 4), ((2, 13, 18, 1), 'linear', 0, 5)],
                         ids=['vol', 'img'])
def test_chunked_drivers_equal_the_whole_call(kom, dtype, shape, kind, p, chunk):
    ndim = len(shape) - 2
    ns = kom.volume if ndim == 3 else kom.image
    ref = reference(dtype, shape, kind, p, 2)
    pred = predictor(kom, kind, p, ndim)
    enc_fn, dec_fn = kom.near.coders(dtype, 2)
    got = ns.encode_chunks(pred, enc_fn, ref['x'], chunk=chunk, padding=p)
    check_encoded(got, ref, 'encode_chunks')
    back = ns.decode_chunks(pred, dec_fn, got[0], got[1], chunk=chunk, padding=p)
    assert back.dtype == np.dtype(dtype) and np.array_equal(back, ref['rec'])


def test_fused_argument_checks(kom):
    """The front door's answers to malformed near requests, before any launch."""
    from kompressor_amd import _lib, _nd
    x = torch.zeros((1, 5, 5, 5, 1), dtype=torch.uint8, device='cuda')
    pred = kom.MeanPredictor(0, 3)
    near8, near16 = _lib.CODER_NEAR_U8, _lib.CODER_NEAR_U16

    def status(t, coder):
        lo, maps, _ = _nd._alloc_encoded(t, _lib.CODER_U8 if t.element_size() == 1 else _lib.CODER_U32, 3)
        try:
            _nd.fused_encode_into(t, pred, coder, lo, maps, 3)
        except _lib.KompressorHipError as e:
            return int(str(e).split('(')[1].split(')')[0])
        return 0

    assert status(x, _lib.coder_near(near8, 127)) == 0
    assert status(x, _lib.CODER_U8 | (5 << 8)) == _lib.KMP_ERR_ARG
    assert status(x, near8) == _lib.KMP_ERR_ARG
    assert status(x, _lib.coder_near(near8, 128)) == _lib.KMP_ERR_ARG
    assert status(x, _lib.coder_near(near16, 1)) == _lib.KMP_ERR_ARG
    assert status(x.view(torch.int8), _lib.coder_near(near16, 1)) == _lib.KMP_ERR_ARG
    x32 = torch.zeros((1, 5, 5, 5, 1), dtype=torch.int32, device='cuda')
    assert status(x32.view(torch.uint32), _lib.coder_near(near16, 1)) == _lib.KMP_ERR_UNSUPPORTED
    assert status(x32, _lib.coder_near(near8, 1)) == _lib.KMP_ERR_UNSUPPORTED


# ---------------------------------------------------------------------------------------------
# the closed loop
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype,delta', [(np.uint16, 2), (np.uint16, 32767), (np.int8, 3), (np.uint8, 1), (np.int16, 100)],
                         ids=['uint16-2', 'uint16-max', 'int8-3', 'uint8-1', 'int16-100'])
@pytest.mark.parametrize('shape,kind,p', [((1, 20, 22, 24, 1), 'mean', 0), ((1, 20, 22, 24, 1), 'linear', 1),
                                          ((2, 13, 17, 1), 'mean', 1), ((2, 13, 17, 1), 'linear', 0)],
                         ids=['vol-mean-p0', 'vol-linear-p1', 'img-mean-p1', 'img-linear-p0'])
def test_encode_pyramid_equals_the_spec(kom, dtype, delta, shape, kind, p):
    ndim = len(shape) - 2
    ns = kom.volume if ndim == 3 else kom.image
    x = NS.noise(shape, dtype, seed=21)
    x[0, ..., 0][tuple(slice(0, s // 2) for s in shape[1:-1])] = \
        NS.noisy_field((1, *[s // 2 for s in shape[1:-1]], 1), dtype, seed=2)[0, ..., 0]
    pred, fn = predictor(kom, kind, p, ndim), spec_fn(kind, p, ndim, dtype)
    for levels in (1, 2, 3):
        want_lo, want_enc, r = NS.encode_pyramid(x, fn, ndim, p, levels, delta)
        lo, enc, restored = kom.near.encode_pyramid(pred, x, levels, delta)
        assert lo.dtype == x.dtype and np.array_equal(lo, want_lo)
        assert len(enc) == levels
        for k, ((maps, dims), (wmaps, wdims)) in enumerate(zip(enc, want_enc)):
            assert tuple(dims) == wdims
            for a, b in zip(maps, wmaps):
                assert a.dtype == b.dtype and np.array_equal(a, b), f'levels {levels}: level {k}'
        assert restored.dtype == x.dtype and np.array_equal(restored, r[0])
        assert np.abs(restored.astype(np.int64) - x.astype(np.int64)).max() <= delta
        # the existing decode_pyramid with the dequantising coder is the decoder
        back = ns.decode_pyramid(pred, kom.near.coders(dtype, delta)[1], lo, enc, padding=p)
        assert np.array_equal(back, restored)
    # torch in, torch out, and the caller's tensor untouched
    xt = torch.from_numpy(x).cuda()
    lo_t, enc_t, rest_t = kom.near.encode_pyramid(pred, xt, 2, delta)
    assert np.array_equal(host(xt), x) and rest_t.is_cuda
    assert np.array_equal(host(rest_t), NS.encode_pyramid(x, fn, ndim, p, 2, delta)[2][0])


def test_encode_pyramid_zero_is_lossless(kom):
    x = NS.noise((1, 9, 10, 11, 1), np.uint16, seed=4)
    pred = kom.MeanPredictor(0, 3)
    lo, enc, restored = kom.near.encode_pyramid(pred, x, 2, 0)
    want_lo, want_enc = kom.volume.encode_pyramid(pred, kom.utils.encode_values_uint16, x, 2, padding=0)
    assert np.array_equal(lo, want_lo) and np.array_equal(restored, x)
    for (maps, dims), (wmaps, wdims) in zip(enc, want_enc):
        assert tuple(dims) == tuple(wdims) and all(np.array_equal(a, b) for a, b in zip(maps, wmaps))


def test_two_encodes_give_identical_bits(kom):
    x = torch.from_numpy(NS.noise((2, 21, 22, 35, 1), np.uint16, seed=8)).cuda()
    pred = kom.MeanPredictor(1, 3)
    runs = [kom.near.encode_pyramid(pred, x, 2, 5) for _ in range(2)]
    assert torch.equal(runs[0][0].view(torch.int16), runs[1][0].view(torch.int16))
    assert torch.equal(runs[0][2].view(torch.int16), runs[1][2].view(torch.int16))
    for (m0, d0), (m1, d1) in zip(runs[0][1], runs[1][1]):
        assert d0 == d1 and all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for a, b in zip(m0, m1))
