"""Time series on the GPU: kmp_code with KMP_CODER_DELTA in both directions and both kernel forms against
the bits of tests/delta_spec.py, ``out == x``, every KMP_ERR_ARG case, the other entry points refusing the
code, and ``kom.delta`` on numpy and CUDA inputs."""

import ctypes

import numpy as np
import pytest
import torch

import delta_spec as D

pytestmark = pytest.mark.gpu

KMP_ERR_ARG = -1
U8, U16, I32, F32, U32, I8, I16 = 0, 1, 2, 3, 4, 5, 6
DELTA = 13
CODE = {np.dtype(np.uint8): U8, np.dtype(np.int8): I8, np.dtype(np.uint16): U16, np.dtype(np.int16): I16,
        np.dtype(np.int32): I32}
TORCH = {np.dtype(np.uint8): torch.uint8, np.dtype(np.int8): torch.int8, np.dtype(np.uint16): torch.uint16,
         np.dtype(np.int16): torch.int16, np.dtype(np.int32): torch.int32}
IDS = [np.dtype(d).name for d in D.DTYPES]
# one element, below / at / above one 16-byte item of every width, no multiple of an item, more than one
# workgroup of either form (2 * 256 * 16 samples are two workgroups of 16-byte items of 8-bit samples)
COUNTS = (1, 3, 15, 16, 17, 4101, 2 * 256 * 16, 2 * 256 * 16 + 5)
OFFSETS = [(p, x, o) for p in (0, 1) for x in (0, 1) for o in (0, 1)]


def uniform(n, dtype, seed):
    info = np.iinfo(dtype)
    a = np.random.default_rng(seed).integers(info.min, int(info.max) + 1, size=n, dtype=np.int64).astype(dtype)
    a[:min(n, 3)] = np.array([info.min, info.max, 0], dtype)[:min(n, 3)]
    return a


def placed(a, off):
    """``a`` on the device, starting ``off`` elements past a 256-byte boundary of a zeroed buffer of its own:
    ``(buffer, index of a[0] in it, the view)``."""
    pad = 256 // a.dtype.itemsize
    buf = torch.zeros((a.size + 2 * pad + 1,), dtype=TORCH[a.dtype], device='cuda')
    at = (-buf.data_ptr() % 256) // a.dtype.itemsize + pad + off
    view = buf[at:at + a.size]
    assert (view.data_ptr() - off * a.dtype.itemsize) % 256 == 0
    view.copy_(torch.from_numpy(a).cuda())
    return buf, at, view


def code(lib, direction, dt, pred, x, out, n=None, coder=DELTA, pred_dt=None):
    from kompressor_amd import _device as dev
    ptr = lambda t: t if t is None or isinstance(t, int) else t.data_ptr()
    return lib.kmp_code(direction, coder, dt if pred_dt is None else pred_dt, ptr(pred), dt, ptr(x),
                        x.numel() if n is None else n, ptr(out), dev.stream())


@pytest.mark.parametrize('direction', (0, 1), ids=('encode', 'decode'))
@pytest.mark.parametrize('dtype', D.DTYPES, ids=IDS)
def test_kmp_code_equals_the_spec(kom, dtype, direction):
    lib = kom._lib.lib
    for n in COUNTS:
        x, p = uniform(n, dtype, seed=n), uniform(n, dtype, seed=n + 1)[::-1].copy()
        want = D.sub(x, p) if direction == 0 else D.add(x, p)
        for off_p, off_x, off_o in OFFSETS:
            _, _, pt = placed(p, off_p)
            _, _, xt = placed(x, off_x)
            obuf, at, ot = placed(np.zeros(n, dtype), off_o)
            assert code(lib, direction, CODE[np.dtype(dtype)], pt, xt, ot) == 0, lib.kmp_last_error()
            assert lib.kmp_last_launch() == b'delta'
            assert np.array_equal(ot.cpu().numpy(), want), (n, off_p, off_x, off_o)
            assert np.array_equal(pt.cpu().numpy(), p) and np.array_equal(xt.cpu().numpy(), x)
            whole = obuf.cpu().numpy()
            assert not whole[:at].any() and not whole[at + n:].any(), (n, off_p, off_x, off_o)


@pytest.mark.parametrize('dtype', D.DTYPES, ids=IDS)
def test_out_may_be_x(kom, dtype):
    lib = kom._lib.lib
    for n in COUNTS:
        x, p = uniform(n, dtype, seed=2 * n), uniform(n, dtype, seed=2 * n + 1)
        for direction, want in ((0, D.sub(x, p)), (1, D.add(x, p))):
            for off in (0, 1):  # the 16-byte form where the count allows it, and the element form
                _, _, pt = placed(p, off)
                xbuf, at, xt = placed(x, off)
                assert code(lib, direction, CODE[np.dtype(dtype)], pt, xt, xt) == 0, lib.kmp_last_error()
                assert np.array_equal(xt.cpu().numpy(), want), (n, direction, off)
                whole = xbuf.cpu().numpy()
                assert not whole[:at].any() and not whole[at + n:].any()


def test_a_sequence_through_the_two_usages(kom):
    """The header's usage: one ENCODE over the frames 1 .. T-1, one DECODE per frame with the frame just restored."""
    lib = kom._lib.lib
    n = uniform(5 * 77, np.int16, seed=9).reshape(5, 77)
    nt = torch.from_numpy(n).cuda()
    d = torch.empty_like(nt)
    d[0] = nt[0]
    assert code(lib, 0, I16, nt[:-1], nt[1:], d[1:]) == 0
    assert np.array_equal(d.cpu().numpy(), D.encode(n))
    for t in range(1, 5):
        assert code(lib, 1, I16, d[t - 1], d[t], d[t]) == 0
    assert np.array_equal(d.cpu().numpy(), n)


def test_argument_errors(kom):
    lib = kom._lib.lib
    a = torch.zeros(64, dtype=torch.int16, device='cuda')
    b = torch.zeros(64, dtype=torch.int16, device='cuda')
    c = torch.zeros(64, dtype=torch.int16, device='cuda')
    w = torch.zeros(64, dtype=torch.int32, device='cuda')

    def refused(status):
        assert status == KMP_ERR_ARG, (status, lib.kmp_last_error())

    assert code(lib, 0, I16, a, b, c) == 0
    for direction in (0, 1):
        refused(code(lib, direction, I16, None, b, c))  # a NULL pred
        refused(code(lib, direction, I16, None, b, c, n=0))  # ... before the count is looked at
        for field in (1, 255, 1 << 15):  # the code carries no field
            refused(code(lib, direction, I16, a, b, c, coder=DELTA | (field << 8)))
        for dt in (F32, U32, 7, 99, -1):  # another dtype
            refused(code(lib, direction, dt, a, b, c, n=8))
        for dt, pdt in ((I16, U16), (U16, I16), (I16, I32), (I32, I16), (U8, I8)):  # two dtypes
            refused(code(lib, direction, dt, a, b, c, n=8, pred_dt=pdt))
        refused(code(lib, direction, I16, a, b, c, n=-1))
        refused(code(lib, direction, I16, a, None, c, n=8))  # null pointers
        refused(code(lib, direction, I16, a, b, None, n=8))
        # misaligned pointers, each array on its own
        refused(code(lib, direction, I16, a.data_ptr() + 1, b, c, n=8))
        refused(code(lib, direction, I16, a, b.data_ptr() + 1, c, n=8))
        refused(code(lib, direction, I16, a, b, c.data_ptr() + 1, n=8))
        for off in (1, 2, 3):
            refused(code(lib, direction, I32, w, w[16:], w.data_ptr() + 128 + off, n=8))
        # out overlaps x in part; out overlaps pred, wholly or in part
        refused(code(lib, direction, I16, a, b, b[1:], n=8))
        refused(code(lib, direction, I16, a, b[1:], b, n=8))
        refused(code(lib, direction, I16, a, b, a, n=8))
        refused(code(lib, direction, I16, a, b, a[7:], n=8))
        refused(code(lib, direction, I16, a[7:], b, a, n=8))
        assert code(lib, direction, I16, a, b, b[8:], n=8) == 0  # adjacent is not overlapping
        assert code(lib, direction, I16, a, b, a[8:], n=8) == 0
        assert code(lib, direction, I16, a, b, c, n=0) == 0  # nothing to do
        assert code(lib, direction, I16, a, None, None, n=0) == 0
    for direction in (2, -1, 13):
        refused(code(lib, direction, I16, a, b, c))
    assert not a.cpu().numpy()[:7].any() and not c.cpu().numpy().any()


def test_other_entry_points_refuse_the_code(kom):
    """The fused codec and the callback path take no delta: KMP_ERR_ARG, nothing launched."""
    from kompressor_amd import _lib, _nd
    lib = _lib.lib
    assert _lib.CODER_DELTA == DELTA
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
    for coder in (DELTA, DELTA | (1 << 8)):
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
    # the Python layers do not know it as a codec coder either
    assert not _nd.coder_fits(DELTA, torch.int16) and not _nd.is_near(DELTA)


@pytest.mark.parametrize('dtype', D.DTYPES, ids=IDS)
def test_kom_delta(kom, dtype):
    for T in (1, 2, 5):
        n = uniform(T * 6 * 7 * 9, dtype, seed=T).reshape(T, 6, 7, 9, 1)
        for K in (None, 1, 2, 3, T):
            want = D.encode(n, K)
            d = kom.delta.encode(n, K)
            assert isinstance(d, np.ndarray) and d.dtype == want.dtype and np.array_equal(d, want), (T, K)
            back = kom.delta.decode(d, dtype, K)
            assert isinstance(back, np.ndarray) and back.dtype == np.dtype(dtype) and np.array_equal(back, n)
            # a CUDA tensor in gives a CUDA tensor out, the same bits
            dt = kom.delta.encode(torch.from_numpy(n).cuda(), K)
            assert isinstance(dt, torch.Tensor) and dt.is_cuda and np.array_equal(dt.cpu().numpy(), want)
            bt = kom.delta.decode(dt, TORCH[np.dtype(dtype)], K)
            assert bt.is_cuda and bt.dtype == TORCH[np.dtype(dtype)] and np.array_equal(bt.cpu().numpy(), n)
            assert np.array_equal(dt.cpu().numpy(), want)  # the decode left its input alone
            assert np.array_equal(kom.delta.decode(d, np.dtype(dtype).name, K), n)


def test_kom_delta_wraps_and_empty(kom):
    n = np.array([0, 65535, 0], np.uint16).reshape(3, 1)
    assert kom.delta.encode(n).reshape(-1).tolist() == [0, -1, 1]
    n = np.array([-32768, 32767, -32768], np.int16).reshape(3, 1)
    assert kom.delta.encode(n).reshape(-1).tolist() == [-32768, -1, 1]
    n = np.array([0, 255, 0], np.uint8).reshape(3, 1)
    assert kom.delta.encode(n).reshape(-1).tolist() == [0, -1, 1]
    for shape in ((0, 4, 5, 1), (3, 0, 5, 1)):
        e = np.zeros(shape, np.int16)
        assert kom.delta.encode(e, 2).shape == shape and kom.delta.decode(e, np.int16, 2).shape == shape


def test_kom_delta_argument_errors(kom):
    n = np.zeros((3, 4), np.int16)
    for bad in (True, False, 0, -1, 2.0, '2', (2,)):
        with pytest.raises(ValueError):
            kom.delta.encode(n, bad)
        with pytest.raises(ValueError):
            kom.delta.decode(n, np.int16, bad)
    for dt in (np.float32, np.uint32, np.int64):
        with pytest.raises(TypeError):
            kom.delta.encode(np.zeros((3, 4), dt))
        with pytest.raises(TypeError):
            kom.delta.decode(n, dt)
    with pytest.raises(TypeError):
        kom.delta.decode(n.view(np.uint16), np.uint16)  # the deltas are the signed type
    with pytest.raises(TypeError):
        kom.delta.decode(n, np.int32)  # ... of the samples' width
