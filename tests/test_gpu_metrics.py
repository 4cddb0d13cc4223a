"""The comparing kernels on the GPU: kmp_code with KMP_CODER_COMPARE against tests/metrics_spec.py for the five
dtypes on both kernels (the vector form at 16-byte aligned pointers and a count that is a multiple of the
item, the element form everywhere else), the partial records and the untouched rest of ``out``, continue
mode, determinism, every KMP_ERR_ARG case, the other entry points refusing the code, and ``kom.metrics``
on numpy and CUDA inputs."""

import ctypes
import math

import numpy as np
import pytest
import torch

import metrics_spec as M
import quant_spec as Q

pytestmark = pytest.mark.gpu

KMP_ERR_ARG = -1
U8, U16, I32, F32, U32, I8, I16 = 0, 1, 2, 3, 4, 5, 6
CODE = {np.dtype(np.float32): F32, np.dtype(np.uint8): U8, np.dtype(np.uint16): U16, np.dtype(np.int8): I8,
        np.dtype(np.int16): I16}
DTYPES = [np.float32, np.uint8, np.uint16, np.int8, np.int16]
IDS = [np.dtype(d).name for d in DTYPES]
COMPARE, CONTINUE = 10, 10 | (1 << 8)
GROUPS, BYTES, THREADS = 1024, 64 * 1025, 256
COUNTS = (1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 4100, 4101)
OFFSETS = ((0, 0), (1, 1), (0, 1))  # elements x and r start past a 256-byte boundary
SENTINEL = 0x5A5A5A5A5A5A5A5A


def item(dtype):
    return 16 // np.dtype(dtype).itemsize


def pair(n, dtype, seed):
    """float32: random bit patterns on both sides (non-finite values, mismatches, huge errors), every
    second element a value with its restored one a few steps away, every fourth kept bit for bit (NaNs and
    infinities among them).  Integers: the full range on both sides, every second a few steps apart."""
    rng = np.random.default_rng(seed)
    if np.dtype(dtype) == np.float32:
        x, r = Q.random_bits(n, seed), Q.random_bits(n, seed + 1)
        vals = rng.uniform(-40, 40, size=n).astype(np.float32)
        x[::2] = vals[::2]
        r[::2] = (vals + rng.integers(-3, 4, size=n).astype(np.float32) * np.float32(2.0 ** -6))[::2]
        r[1::4] = x[1::4]
        return x, r
    info = np.iinfo(dtype)
    x = rng.integers(info.min, int(info.max) + 1, size=n, dtype=np.int64)
    r = rng.integers(info.min, int(info.max) + 1, size=n, dtype=np.int64)
    r[::2] = np.clip(x[::2] + rng.integers(-3, 4, size=x[::2].size), info.min, info.max)
    return x.astype(dtype), r.astype(dtype)


def exact_pair(n, seed):
    """float32 values that are integer multiples of 2^-20 below 2^10 whose errors keep every float64 sum
    exact: one half multiples of 2^-10 below 2^10 restored up to 32 such steps away (e^2 <= 2^-10, a multiple
    of 2^-20), the other half multiples of 2^-20 below 8 restored up to 63 steps away (e^2 < 2^-28, a
    multiple of 2^-40).  Any sum of up to 2^20 such squares is a multiple of 2^-40 below 2^11: 51 bits."""
    rng = np.random.default_rng(seed)
    k = rng.integers(-(2 ** 20) + 64, 2 ** 20 - 64, size=n)
    x = (k * 2.0 ** -10).astype(np.float32)
    r = ((k + rng.integers(-32, 33, size=n)) * 2.0 ** -10).astype(np.float32)
    k2 = rng.integers(-(2 ** 23) + 64, 2 ** 23 - 64, size=n)
    x[1::2] = (k2 * 2.0 ** -20).astype(np.float32)[1::2]
    r[1::2] = ((k2 + rng.integers(-63, 64, size=n)) * 2.0 ** -20).astype(np.float32)[1::2]
    assert np.array_equal(x.astype(np.float64) * 2 ** 20, np.rint(x.astype(np.float64) * 2 ** 20)) and np.abs(x).max() < 2 ** 10
    return x, r


def placed(a, off):
    """``a``'s bytes on the device, starting ``off`` elements past a 256-byte boundary: (keep-alive, address)."""
    a = np.ascontiguousarray(a)
    buf = torch.zeros((a.nbytes + 64,), dtype=torch.uint8, device='cuda')
    assert buf.data_ptr() % 256 == 0
    lo = off * a.dtype.itemsize
    buf[lo:lo + a.nbytes] = torch.from_numpy(a.reshape(-1).view(np.uint8)).cuda()
    return buf, buf.data_ptr() + lo


def fresh_out():
    return torch.full((BYTES // 8,), SENTINEL, dtype=torch.int64, device='cuda')


def run(lib, coder, x, r, offs=(0, 0), out=None, n=None):
    """One call: (status, out buffer)."""
    from kompressor_amd import _device as dev
    xb, xp = placed(x, offs[0])
    rb, rp = placed(r, offs[1])
    out = fresh_out() if out is None else out
    code = CODE[x.dtype]
    st = lib.kmp_code(0, coder, code, rp, code, xp, x.size if n is None else n, out.data_ptr(), dev.stream())
    torch.cuda.synchronize()
    return st, out


def groups(n, dtype, offs):
    V = item(dtype)
    vec = n % V == 0 and all(o * np.dtype(dtype).itemsize % 16 == 0 for o in offs)
    return min(GROUPS, -(-(n // V if vec else n) // THREADS))


def check_words(words, x, r, G, start=None, before=0):
    """The record and the partials of one call against the spec (``start``: the record continued, of
    ``before`` elements)."""
    is_float = x.dtype == np.float32
    own = M.record(x, r)
    want = own if start is None else M.fold(start, own)
    got = M.from_words(words[:8], is_float)
    exact = ('count', 'mismatch', 'max_abs', 'x_min', 'x_max') + (() if is_float else ('sse',))
    assert {k: got[k] for k in exact} == {k: want[k] for k in exact}
    assert words[6] == words[7] == 0
    n = before + x.size
    if is_float:
        assert M.sse_ok(got['sse'], n, want['sse']), (got['sse'], want['sse'])
        # the bit patterns of the exact float fields, the sign of a zero included
        assert np.array_equal(words[[2, 4, 5]], M.words(want, True)[[2, 4, 5]])
    else:
        assert np.array_equal(words[:8], M.words(want, False))
    # the partial records of the workgroups that ran fold to the call's own record; the rest is untouched
    part = {'count': 0, 'mismatch': 0, 'max_abs': 0.0, 'sse': 0.0 if is_float else 0, 'x_min': math.inf, 'x_max': -math.inf}
    for g in range(G):
        w = words[8 * (1 + g):8 * (2 + g)]
        assert w[6] == w[7] == 0
        part = M.fold(part, M.from_words(w, is_float))
    assert {k: part[k] for k in exact} == {k: own[k] for k in exact}
    if is_float:
        assert M.sse_ok(part['sse'], x.size, own['sse'])
    assert (words[8 * (1 + G):] == np.uint64(SENTINEL)).all()
    return want


def words_of(out):
    return out.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_kmp_code_equals_the_spec(kom, dtype):
    lib = kom._lib.lib
    for n in COUNTS:
        x, r = pair(n, dtype, seed=7 * n)
        for offs in OFFSETS:
            st, out = run(lib, COMPARE, x, r, offs)
            assert st == 0, lib.kmp_last_error()
            assert lib.kmp_last_launch() == b'compare'
            check_words(words_of(out), x, r, groups(n, dtype, offs))


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_grid_stride_trips_and_a_ragged_tail(kom, dtype):
    """Every thread of every workgroup makes a second trip: the element kernel at GROUPS * 256 * item + item
    + 1 elements (aligned and not), the vector kernel at 2 * GROUPS * 256 + 5 items."""
    lib = kom._lib.lib
    V = item(dtype)
    n = GROUPS * THREADS * V + V + 1
    x, r = pair(n, dtype, seed=11)
    for offs in ((0, 0), (1, 1)):
        st, out = run(lib, COMPARE, x, r, offs)
        assert st == 0 and groups(n, dtype, offs) == GROUPS
        check_words(words_of(out), x, r, GROUPS)
    nv = (2 * GROUPS * THREADS + 5) * V
    x, r = pair(nv, dtype, seed=12)
    st, out = run(lib, COMPARE, x, r)
    assert st == 0
    check_words(words_of(out), x, r, GROUPS)


def test_exact_sums_are_bit_equal_in_any_order(kom):
    """On :func:`exact_pair` every float64 partial sum is exact, so the device's ``sse`` is the spec's bits
    whatever its order -- on both kernels, and over three slabs in continue mode."""
    lib = kom._lib.lib
    for n, offs in ((1 << 20, (0, 0)), ((1 << 20) - 3, (1, 1)), (4100, (0, 0)), (4101, (0, 1))):
        x, r = exact_pair(n, seed=n)
        st, out = run(lib, COMPARE, x, r, offs)
        assert st == 0
        assert np.array_equal(words_of(out)[:8], M.words(M.record(x, r), True))
    x, r = exact_pair(70000, seed=5)
    out = None
    for k, (a, b) in enumerate(((0, 1000), (1000, 66003), (66003, 70000))):
        st, out = run(lib, CONTINUE if k else COMPARE, x[a:b], r[a:b], (a % 4 != 0, a % 4 != 0), out)
        assert st == 0
    assert np.array_equal(words_of(out)[:8], M.words(M.record(x, r), True))


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_continue_mode(kom, dtype):
    lib = kom._lib.lib
    x, r = pair(9000, dtype, seed=21)
    cuts, out, start = (0, 37, 37 + 16 * 300, 9000), None, None
    for k, (a, b) in enumerate(zip(cuts, cuts[1:])):
        offs = (0, 0) if k == 1 else (1, 1)
        st, out = run(lib, CONTINUE if k else COMPARE, x[a:b], r[a:b], offs, out)
        assert st == 0, lib.kmp_last_error()
        w = words_of(out)
        G = groups(b - a, dtype, offs)
        # partials of an earlier, larger call stay where they are: only this call's are judged
        w = np.concatenate([w[:8 * (1 + G)], np.full(w.size - 8 * (1 + G), SENTINEL, np.uint64)])
        start = check_words(w, x[a:b], r[a:b], G, start, before=a)
    final = M.from_words(words_of(out)[:8], dtype == np.float32)
    want = M.record(x, r)
    for k in ('count', 'mismatch', 'max_abs', 'x_min', 'x_max'):
        assert final[k] == want[k]
    if dtype == np.float32:
        assert M.sse_ok(final['sse'], x.size, want['sse'])
    else:
        assert np.array_equal(words_of(out)[:8], M.words(want, False))
    # n == 0 touches nothing, in either mode
    before = words_of(out).copy()
    for coder in (COMPARE, CONTINUE):
        st, out = run(lib, coder, x[:4], r[:4], (0, 0), out, n=0)
        assert st == 0 and np.array_equal(words_of(out), before)


@pytest.mark.parametrize('dtype', [np.float32, np.uint16], ids=['float32', 'uint16'])
def test_two_calls_give_identical_buffers(kom, dtype):
    lib = kom._lib.lib
    for n, offs in ((4101, (1, 1)), (300000 * item(dtype) // 4, (0, 0))):
        x, r = pair(n, dtype, seed=n)
        a = words_of(run(lib, COMPARE, x, r, offs)[1])
        b = words_of(run(lib, COMPARE, x, r, offs)[1])
        assert np.array_equal(a, b)


def test_argument_errors(kom):
    from kompressor_amd import _device as dev
    lib = kom._lib.lib
    x = torch.zeros(64, dtype=torch.float32, device='cuda')
    r = torch.zeros(64, dtype=torch.float32, device='cuda')
    out = fresh_out()

    def code(direction, coder, pc, pred, xc, xx, n, o):
        return lib.kmp_code(direction, coder, pc, pred, xc, xx, n, o, dev.stream())

    def refused(status):
        assert status == KMP_ERR_ARG, (status, lib.kmp_last_error())

    X, R, O = x.data_ptr(), r.data_ptr(), out.data_ptr()
    assert code(0, COMPARE, F32, R, F32, X, 8, O) == 0
    for coder in (COMPARE, CONTINUE):
        refused(code(0, coder, F32, None, F32, X, 8, O))  # no restored array
        refused(code(0, coder, F32, None, F32, X, 0, O))  # ... before the count is looked at
        refused(code(1, coder, F32, R, F32, X, 8, O))     # KMP_DECODE
        refused(code(2, coder, F32, R, F32, X, 8, O))
        for xc, pc in ((F32, U8), (U8, F32), (U16, I16), (I8, U8), (I32, I32), (U32, U32), (99, 99), (-1, -1)):
            refused(code(0, coder, pc, R, xc, X, 8, O))   # differing or unsupported dtypes
        for mis in (1, 2, 4, 7):
            refused(code(0, coder, F32, R, F32, X, 8, O + mis))  # a misaligned out
        for xc in (U16, I16):
            refused(code(0, coder, xc, R, xc, X, 1 << 32, O))  # the u64 sse could overflow
            refused(code(0, coder, xc, R, xc, X, (1 << 40) + 8, O))
        refused(code(0, coder, F32, R, F32, X, -1, O))
        refused(code(0, coder, F32, R, F32, None, 8, O))  # null pointers
        refused(code(0, coder, F32, R, F32, X, 8, None))
        assert code(0, coder, F32, R, F32, None, 0, None) == 0  # nothing to do
    for field in (2, 3, 127, 255, 256, 1 << 20):
        refused(code(0, 10 | (field << 8), F32, R, F32, X, 8, O))
        refused(code(0, 10 | (field << 8), F32, R, F32, X, 0, O))
    refused(code(0, -10, F32, R, F32, X, 8, O))
    refused(code(0, 11, F32, R, F32, X, 8, O))
    torch.cuda.synchronize()
    # nothing was launched by a refusal: the buffer is the first call's
    w = words_of(out)
    assert w[0] == 8 and (w[16:] == np.uint64(SENTINEL)).all()


def test_other_entry_points_refuse_the_code(kom):
    """The fused codec and the callback path take no comparison: KMP_ERR_ARG, nothing launched."""
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
    for coder in (_lib.CODER_COMPARE, _lib.coder_compare(True)):
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


def close(got, want, n):
    """A ``metrics.compare`` result against the spec's: exact but for what follows from the float ``sse``."""
    for k in ('count', 'mismatch', 'max_abs_error', 'value_range', 'peak'):
        assert got[k] == want[k], k
    tol = n * 2.0 ** -51
    assert abs(got['mse'] - want['mse']) <= tol * want['mse'] and abs(got['rmse'] - want['rmse']) <= tol * want['rmse']
    assert abs(got['nrmse'] - want['nrmse']) <= tol * want['nrmse'] and abs(got['psnr'] - want['psnr']) <= 1e-9


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_metrics_compare(kom, dtype):
    if dtype == np.float32:
        x = Q.spec_field()[0, :9]
        n, exc = Q.quantise(x, -7)
        r = Q.restore(n, -7, exc)
    else:
        x, r = pair(5 * 7 * 11, dtype, seed=2)
        x, r = x.reshape(5, 7, 11), r.reshape(5, 7, 11)
    for peak in (None, 100.0):
        want = M.compare(x, r, peak)
        got = kom.metrics.compare(x, r, peak)
        if dtype != np.float32:
            assert got == want
        close(got, want, x.size)
        tx, tr = torch.from_numpy(x.copy()).cuda(), torch.from_numpy(r.copy()).cuda()
        assert kom.metrics.compare(tx, tr, peak) == got                 # CUDA tensors in
        assert kom.metrics.compare(x, tr, peak) == got                  # or one of each
    words = kom.metrics.record_words(kom.metrics.d_compare(tx, tr))
    assert kom.metrics.summary(words, dtype) == kom.metrics.compare(x, r)
    # passing the buffer back in continues it
    buf = kom.metrics.d_compare(tx.reshape(-1)[:100], tr.reshape(-1)[:100])
    assert kom.metrics.d_compare(tx.reshape(-1)[100:], tr.reshape(-1)[100:], buf) is buf
    close(kom.metrics.summary(kom.metrics.record_words(buf), dtype), M.compare(x, r), x.size)
    empty = kom.metrics.d_compare(tx[:0], tr[:0])
    assert kom.metrics.summary(kom.metrics.record_words(empty), dtype) == M.compare(x[:0], r[:0])
