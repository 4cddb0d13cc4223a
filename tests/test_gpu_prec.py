"""The relative-error float32 quantisers on the GPU: kmp_code with KMP_CODER_PREC codes in both
directions against the bits of tests/prec_spec.py, every KMP_ERR_ARG case, the other entry points
refusing the codes, and ``kom.quant.quantise_rel`` / ``restore_rel`` on numpy and CUDA inputs."""

import ctypes

import numpy as np
import pytest
import torch

import prec_spec as P

pytestmark = pytest.mark.gpu

KMP_ERR_ARG = -1
F32, I32, U32, I16, U16 = 3, 2, 4, 6, 1
PCODE = {np.dtype(np.int16): 8, np.dtype(np.int32): 9}
NCODE = {np.dtype(np.int16): I16, np.dtype(np.int32): I32}
TORCH = {np.dtype(np.int16): torch.int16, np.dtype(np.int32): torch.int32, np.dtype(np.float32): torch.float32}
COUNTS = (1, 3, 4, 5, 7, 8, 9, 4097)
MS = (0, 7, 8, 22)


def parg(dtype, m):
    return PCODE[np.dtype(dtype)] | ((m + 1) << 8)


def placed(a, off):
    """``a`` on the device in a buffer of its own, starting ``off`` elements into it."""
    buf = torch.zeros((a.size + off,), dtype=TORCH[a.dtype], device='cuda')
    buf[off:] = torch.from_numpy(a).cuda()
    return buf, buf[off:]


def samples(n, m, dtype, seed):
    """Random bit patterns, values of a few units, and the known answers."""
    x = P.random_bits(n, seed)
    x[::2] = np.random.default_rng(seed + 1).uniform(-4, 4, size=n).astype(np.float32)[::2]
    ka = P.known_answers(m, dtype)[0]
    k = min(n, ka.size)
    x[n - k:] = ka[:k]
    return x


def code(lib, direction, coder, x_code, x, out, pred=None, n=None):
    from kompressor_amd import _device as dev
    return lib.kmp_code(direction, coder, 0, pred, x_code, x.data_ptr() if x is not None else None,
                        x.numel() if n is None else n, out.data_ptr() if out is not None else None, dev.stream())


def bits_of(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize('m', MS)
@pytest.mark.parametrize('dtype', [np.int16, np.int32], ids=['int16', 'int32'])
def test_kmp_code_equals_the_spec(kom, dtype, m):
    lib = kom._lib.lib
    for n in COUNTS:
        x = samples(n, m, dtype, seed=3 * n)
        want = P.encode_bits(x, m, dtype)
        ints = np.random.default_rng(n).integers(np.iinfo(dtype).min, int(np.iinfo(dtype).max) + 1, size=n,
                                                 dtype=np.int64).astype(dtype)
        ints[:min(n, 4)] = np.array([np.iinfo(dtype).min, 0, -1, np.iinfo(dtype).max], dtype)[:min(n, 4)]
        back = P.dequant(ints, m)
        for off_in, off_out in ((0, 0), (1, 1), (1, 0), (0, 1)):
            _, xt = placed(x, off_in)
            obuf, ot = placed(np.zeros(n, dtype), off_out)
            assert code(lib, 0, parg(dtype, m), F32, xt, ot) == 0, lib.kmp_last_error()
            assert np.array_equal(ot.cpu().numpy(), want), (n, off_in, off_out)
            assert off_out == 0 or int(obuf[0].item()) == 0
            _, it = placed(ints, off_in)
            fbuf, ft = placed(np.zeros(n, np.float32), off_out)
            assert code(lib, 1, parg(dtype, m), NCODE[np.dtype(dtype)], it, ft) == 0, lib.kmp_last_error()
            assert np.array_equal(bits_of(ft), back.view(np.uint32)), (n, off_in, off_out)
            assert off_out == 0 or int(fbuf[0].item()) == 0


def test_known_answers_and_the_guarantee(kom):
    lib = kom._lib.lib
    for dtype in (np.int16, np.int32):
        for m in (0, 6, 7, 8, 22):
            x, n_want, exc_want = P.known_answers(m, dtype)
            x = np.concatenate([x, P.random_bits(4096 - x.size, seed=m)])
            xt = torch.from_numpy(x).cuda()
            ot = torch.zeros(x.size, dtype=TORCH[np.dtype(dtype)], device='cuda')
            assert code(lib, 0, parg(dtype, m), F32, xt, ot) == 0
            got = ot.cpu().numpy()
            assert np.array_equal(got, P.encode_bits(x, m, dtype))
            k = n_want.size
            assert np.array_equal(got[:k] == np.iinfo(dtype).min, exc_want)
            assert np.array_equal(got[:k][~exc_want].astype(np.int64), n_want[~exc_want])
            ft = torch.zeros(x.size, dtype=torch.float32, device='cuda')
            assert code(lib, 1, parg(dtype, m), NCODE[np.dtype(dtype)], ot, ft) == 0
            r = ft.cpu().numpy()
            ok = got != np.iinfo(dtype).min
            assert np.isfinite(r[ok]).all() and P.rel_errors(x[ok], r[ok]).max(initial=0.0) <= 2.0 ** -(m + 1)
            # restoring is idempotent: the restored values quantise to the same integers
            assert code(lib, 0, parg(dtype, m), F32, ft, ot) == 0
            assert np.array_equal(ot.cpu().numpy()[ok], got[ok])


def test_argument_errors(kom):
    lib = kom._lib.lib
    x = torch.zeros(8, dtype=torch.float32, device='cuda')
    n16 = torch.zeros(8, dtype=torch.int16, device='cuda')
    n32 = torch.zeros(8, dtype=torch.int32, device='cuda')

    def refused(status):
        assert status == KMP_ERR_ARG, (status, lib.kmp_last_error())

    refused(code(lib, 0, parg(np.int16, 6), F32, x, n16, pred=x.data_ptr()))  # a prediction
    refused(code(lib, 1, parg(np.int32, 6), I32, n32, x, pred=n32.data_ptr()))
    refused(code(lib, 0, parg(np.int16, 6), F32, x, n16, pred=x.data_ptr(), n=0))  # before the count is looked at
    for field in (0, 24, 25, 127, 255, 256, 1 << 20):  # the field is m + 1, in [1, 23]
        for c in (8, 9):
            refused(code(lib, 0, c | (field << 8), F32, x, n32))
            refused(code(lib, 1, c | (field << 8), I16 if c == 8 else I32, n16 if c == 8 else n32, x))
            refused(code(lib, 0, c | (field << 8), F32, None, None, n=0))
    for xc in (I32, U32, I16, U16, 0, 5, 99):  # an encode takes float32
        refused(code(lib, 0, parg(np.int16, 6), xc, x, n16))
        refused(code(lib, 0, parg(np.int32, 6), xc, x, n32))
    for xc in (F32, I32, U16, U32):  # a decode takes the code's own integer dtype
        refused(code(lib, 1, parg(np.int16, 6), xc, n16, x))
    for xc in (F32, I16, U32, U16):
        refused(code(lib, 1, parg(np.int32, 6), xc, n32, x))
    refused(code(lib, 2, parg(np.int32, 6), F32, x, n32))  # direction
    refused(code(lib, 0, parg(np.int32, 6), F32, x, n32, n=-1))
    refused(code(lib, 0, parg(np.int32, 6), F32, None, n32, n=8))  # null pointers
    refused(code(lib, 0, parg(np.int32, 6), F32, x, None, n=8))
    for c in (parg(np.int16, 0), parg(np.int32, 22)):  # nothing to do
        assert code(lib, 0, c, F32, None, None, n=0) == 0
        assert code(lib, 1, c, I16 if c & 0xff == 8 else I32, None, None, n=0) == 0
    refused(code(lib, 0, 8, F32, x, n32))  # a bare code: field 0
    refused(code(lib, 0, 9, F32, x, n32))
    refused(code(lib, 0, 10 | (1 << 8), F32, x, n32))  # no such coder
    refused(code(lib, 0, -8, F32, x, n32))


def test_other_entry_points_refuse_the_codes(kom):
    """The fused codec and the callback path take no quantiser: KMP_ERR_ARG, nothing launched."""
    from kompressor_amd import _lib, _nd
    lib = _lib.lib
    x = torch.zeros((1, 5, 5, 5, 1), dtype=torch.int16, device='cuda')
    lowres, maps, dims = _nd._alloc_encoded(x, _lib.CODER_U16, 3)
    probe = _lib.Predictor(0, 0, None, None)
    need = int(lib.kmp_volume_workspace_bytes(I16, 1, 5, 5, 5, 1, ctypes.byref(probe)))
    ws = torch.zeros((max(need, 8),), dtype=torch.uint8, device='cuda')
    dims_out = (ctypes.c_int32 * 3)()
    img = torch.zeros((1, 5, 5, 1), dtype=torch.int16, device='cuda')
    ilow, imaps, idims = _nd._alloc_encoded(img, _lib.CODER_U16, 2)
    probe2 = _lib.Predictor(0, 0, None, None)
    spare = [torch.zeros(256, dtype=torch.int16, device='cuda') for _ in range(7)]
    for coder in (_lib.coder_prec(_lib.CODER_PREC_I16, 0), _lib.coder_prec(_lib.CODER_PREC_I32, 22), 8, 9):
        st = [lib.kmp_volume_encode(I16, x.data_ptr(), 1, 5, 5, 5, 1, ctypes.byref(probe), coder, lowres.data_ptr(),
                                    _lib.ptrs(maps), dims_out, None, ws.data_ptr(), need, None),
              lib.kmp_volume_decode(I16, lowres.data_ptr(), _lib.ptrs(maps), 1, *lowres.shape[1:4], 1,
                                    _lib.i32xn(dims), ctypes.byref(probe), coder, x.data_ptr(), None, ws.data_ptr(),
                                    need, None),
              lib.kmp_image_encode(I16, img.data_ptr(), 1, 5, 5, 1, ctypes.byref(probe2), coder, ilow.data_ptr(),
                                   _lib.ptrs(imaps), dims_out, None, ws.data_ptr(), need, None),
              lib.kmp_image_decode(I16, ilow.data_ptr(), _lib.ptrs(imaps), 1, *ilow.shape[1:3], 1, _lib.i32xn(idims),
                                   ctypes.byref(probe2), coder, img.data_ptr(), None, ws.data_ptr(), need, None),
              lib.kmp_encode_with_predictions(3, I16, coder, x.data_ptr(), 1, _lib.i64x3((5, 5, 5)), 1, _lib.ptrs(spare),
                                              lowres.data_ptr(), _lib.ptrs(maps), None),
              lib.kmp_encode_with_predictions_typed(3, I16, coder, F32, x.data_ptr(), 1, _lib.i64x3((5, 5, 5)), 1,
                                                    _lib.ptrs(spare), lowres.data_ptr(), _lib.ptrs(maps), None),
              lib.kmp_decode_with_predictions(3, I16, coder, lowres.data_ptr(), _lib.ptrs(maps), 1,
                                              _lib.i64x3(lowres.shape[1:4]), 1, _lib.i32xn(dims), _lib.ptrs(spare),
                                              x.data_ptr(), None),
              lib.kmp_decode_with_predictions_typed(3, I16, coder, F32, lowres.data_ptr(), _lib.ptrs(maps), 1,
                                                    _lib.i64x3(lowres.shape[1:4]), 1, _lib.i32xn(dims), _lib.ptrs(spare),
                                                    x.data_ptr(), None)]
        assert st == [KMP_ERR_ARG] * 8, (coder, st, lib.kmp_last_error())


def bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _decades(shape, seed, lo, hi):
    """Both signs, magnitudes log-uniform in ``[lo, hi)``."""
    rng = np.random.default_rng(seed)
    return (rng.choice([-1.0, 1.0], size=shape) * np.exp(rng.uniform(np.log(lo), np.log(hi), size=shape))).astype(np.float32)


def _with_exceptions(a):
    f = a.reshape(-1)
    f[[0, 5, 17, f.size - 1]] = [np.nan, np.inf, -np.inf, 3.4028235e38]  # the last one rounds up to infinity
    f[40:44].view(np.uint32)[:] = [0x7fc00001, 0xffc12345, 0x7f800001, 0xff800000]  # NaN payloads, -inf
    return a


# (the mantissa bits asked for as a bound, the array): at m = 8 an array below 2.0 in magnitude fits int16
CASES = {
    'int16-m6': lambda: (1e-2, _decades((2, 7, 9, 11, 1), 1, 1e-6, 1e6)),
    'int16-m8': lambda: (2.0 ** -9, _decades((2, 7, 9, 11, 1), 2, 1e-6, 1.99)),
    'int32-m8': lambda: (2.0 ** -9, _decades((2, 7, 9, 11, 1), 3, 1e-6, 1e6)),
    'int32-m22': lambda: (2.0 ** -23, _decades((3, 8, 13, 1), 4, 1e-3, 1e3)),
    'int16-m6-exceptions': lambda: (1e-2, _with_exceptions(_decades((3, 8, 13, 1), 5, 1e-6, 1e6))),
    'int16-m8-exceptions': lambda: (2.0 ** -9, _with_exceptions(_decades((3, 8, 13, 1), 6, 1e-6, 1.99))),
    'int32-m9-exceptions': lambda: (1e-3, _with_exceptions(_decades((3, 8, 13, 1), 7, 1e-6, 1e6))),
    'int16-m0-all-exceptions': lambda: (0.5, np.full((1, 4, 5, 6, 1), np.nan, np.float32)),
    'int16-m9-empty': lambda: (1e-3, np.zeros((0, 4, 5, 1), np.float32)),
}


@pytest.mark.parametrize('case', list(CASES))
def test_quantise_rel_restore_rel(kom, case):
    rel_error, x = CASES[case]()
    m = P.mantissa_bits(rel_error)
    assert f'm{m}' in case.split('-')
    n_want, exc_want = P.quantise(x, m)
    assert n_want.dtype == np.dtype(case.split('-')[0])
    assert (exc_want is None) == ('exceptions' not in case)
    n, exc = kom.quant.quantise_rel(x, rel_error)
    assert isinstance(n, np.ndarray) and n.dtype == n_want.dtype and np.array_equal(n, n_want)
    if exc_want is None:
        assert exc is None
    else:
        assert exc[0].dtype == np.int64 and exc[1].dtype == np.uint32
        assert np.array_equal(exc[0], exc_want[0]) and np.array_equal(exc[1], exc_want[1])
        assert np.all(np.diff(exc[0]) > 0) and not n.reshape(-1)[exc[0]].any()
    back = kom.quant.restore_rel(n, m, exc)
    assert isinstance(back, np.ndarray) and bits_equal(back, P.restore(n_want, m, exc_want))
    ok = np.ones(x.size, bool)
    if exc is not None:
        ok[exc[0]] = False
        assert np.array_equal(back.reshape(-1).view(np.uint32)[~ok], x.reshape(-1).view(np.uint32)[~ok])
    assert P.rel_errors(x.reshape(-1)[ok], back.reshape(-1)[ok]).max(initial=0) <= kom.quant.effective_rel(rel_error)
    # a CUDA tensor in gives CUDA tensors out, the same bits; and again: repeatable
    for _ in range(2):
        nt, et = kom.quant.quantise_rel(torch.from_numpy(x).cuda(), rel_error)
        assert isinstance(nt, torch.Tensor) and nt.is_cuda and np.array_equal(nt.cpu().numpy(), n)
        if exc is None:
            assert et is None
        else:
            assert et[0].is_cuda and et[0].dtype == torch.int64 and et[1].dtype == torch.uint32
            assert np.array_equal(et[0].cpu().numpy(), exc[0])
            assert np.array_equal(et[1].view(torch.int32).cpu().numpy().view(np.uint32), exc[1])
        bt = kom.quant.restore_rel(nt, m, et)
        assert isinstance(bt, torch.Tensor) and bt.is_cuda and bits_equal(bt.cpu().numpy(), back)


def test_quantised_arrays_go_through_the_lossless_codec(kom):
    x = P.decades_field()[:, :9, :10, :13]
    n, exc = kom.quant.quantise_rel(x, 1e-2)
    assert n.dtype == np.int16 and exc is None
    pred = kom.MeanPredictor(0, 3)
    lo, enc = kom.volume.encode(pred, kom.volume.encode_values_int16, n)
    assert np.array_equal(kom.volume.decode(pred, kom.volume.decode_values_int16, lo, enc), n)


def test_restore_rel_rejects_bad_exceptions(kom):
    n = np.zeros(6, np.int16)
    with pytest.raises(ValueError):
        kom.quant.restore_rel(n, 6, (np.array([6], np.int64), np.array([1], np.uint32)))
    with pytest.raises(ValueError):
        kom.quant.restore_rel(n, 6, (np.array([-1], np.int64), np.array([1], np.uint32)))
    with pytest.raises(ValueError):
        kom.quant.restore_rel(n, 6, (np.array([1, 2], np.int64), np.array([1], np.uint32)))
