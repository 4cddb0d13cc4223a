"""The SSIM kernels on the GPU: kmp_code with KMP_CODER_SSIM against tests/ssim_spec.py -- the five dtypes on
images and volumes, every spatial extent around the window and around the tile, widths that defeat and that
allow 16-byte reads, offset pointers, items at very different levels, non-finite float32 values, the partial
records and the untouched rest of ``out``, determinism, a graph replay, malformed requests, every KMP_ERR_ARG
case, and ``kom.metrics.ssim`` on numpy and CUDA inputs.

Tolerances (ssim_spec.py): integer moments are exact, so the mean and the minimum stand within 2^-40 of the
spec's; float32 data lies within 2 L of the base, which bounds a window's error by about 4e-11: 1e-9."""

import ctypes
import math

import numpy as np
import pytest
import torch

import ssim_spec as S
import test_gpu_metrics as G

pytestmark = pytest.mark.gpu

KMP_ERR_ARG = -1
SSIM = 14
DTYPES = G.DTYPES
IDS = G.IDS
SENTINEL = G.SENTINEL


def consts():
    from kompressor_amd import _lib
    return _lib


def field(shape, dtype, seed, levels=None):
    """``(x, r)`` of ``shape = (N, D, H, W)``: smooth waves plus noise, restored a little off.  ``levels``: one
    offset per item as a fraction of the dtype's range (float32: of 100.0)."""
    rng = np.random.default_rng(seed)
    N, D, H, W = shape
    z, y, w = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing='ij')
    wave = np.sin(0.7 * w + 0.3 * y) + np.cos(0.5 * y - 0.4 * z) + 0.5 * np.sin(0.9 * z + 0.2 * w)
    x = wave[None] * rng.uniform(0.5, 1.5, size=(N, 1, 1, 1)) + 0.3 * rng.standard_normal(shape)
    e = 0.1 * rng.standard_normal(shape)
    if np.dtype(dtype) == np.float32:
        off = np.zeros(N) if levels is None else 100.0 * np.asarray(levels, np.float64)
        x = x + off[:, None, None, None]
        return x.astype(np.float32), (x + e).astype(np.float32)
    info = np.iinfo(dtype)
    span = float(info.max) - float(info.min)
    amp = span / 16
    mid = np.full(N, 0.5) if levels is None else np.asarray(levels, np.float64)
    centre = (info.min + mid * span)[:, None, None, None]
    xi = np.clip(np.rint(centre + amp * x), info.min, info.max)
    ri = np.clip(np.rint(centre + amp * (x + e)), info.min, info.max)
    return xi.astype(dtype), ri.astype(dtype)


def request_words(dims, c1, c2, base):
    q = np.zeros(8, np.int64)
    q[:3] = dims
    q[3:6] = np.array([c1, c2, base], np.float64).view(np.int64)
    return q


def fresh_out(request):
    out = torch.full((consts().SSIM_BYTES // 8,), SENTINEL, dtype=torch.int64, device='cuda')
    out[8:16] = torch.from_numpy(np.asarray(request, np.int64)).cuda()
    return out


def frame(x, peak=None):
    """``(request for the default frame of x, peak, base)``."""
    L, base = S.default_frame(x)
    L = L if peak is None else float(peak)
    return request_words(x.shape[1:], (0.01 * L) ** 2, (0.03 * L) ** 2, base), L, base


def run(lib, x, r, request, offs=(0, 0), n=None, coder=SSIM):
    """One call on the ``(N, D, H, W)`` arrays: (status, the words of ``out``)."""
    from kompressor_amd import _device as dev
    xb, xp = G.placed(x, offs[0])
    rb, rp = G.placed(r, offs[1])
    out = fresh_out(request)
    code = G.CODE[x.dtype]
    st = lib.kmp_code(0, coder, code, rp, code, xp, x.size if n is None else n, out.data_ptr(), dev.stream())
    torch.cuda.synchronize()
    return st, out.cpu().numpy().view(np.uint64)


def check_words(words, x, r, request, peak=None):
    """The record, the request and the partial records of one call against the spec."""
    want = S.ssim(x, r, peak)
    tol = S.TOL_F32 if x.dtype == np.float32 else S.TOL_INT
    f = words.view(np.float64)
    assert (int(words[0]), int(words[1])) == (want['windows'], want['skipped'])
    assert words[4] == 0 and (words[5:8] == 0).all()
    assert np.array_equal(words[8:16].view(np.int64), request)  # the request is only read
    if want['windows']:
        got = f[2] / want['windows']
        print(f'{x.dtype.name} {x.shape}: ssim {got!r} (spec {want["ssim"]!r}, gap {abs(got - want["ssim"]):.3g}), '
              f'min {f[3]!r} (gap {abs(f[3] - want["min_ssim"]):.3g}), windows {want["windows"]}, skipped {want["skipped"]}')
        assert abs(got - want['ssim']) <= tol and abs(f[3] - want['min_ssim']) <= tol
    else:
        assert f[2] == 0.0 and f[3] == math.inf
    # the partial records of the workgroups that ran fold to the record; the rest is untouched
    groups = consts().ssim_groups(x.size)
    part = words[16:16 + 8 * groups].reshape(groups, 8)
    assert int(part[:, 0].sum()) == want['windows'] and int(part[:, 1].sum()) == want['skipped']
    assert (part[:, 4:] == 0).all()
    pf = part.view(np.float64)
    assert pf[:, 3].min() == f[3]
    assert abs(math.fsum(pf[:, 2].tolist()) - f[2]) <= max(1, want['windows']) * 2.0 ** -50 * max(1.0, abs(f[2]))
    assert (words[16 + 8 * groups:] == np.uint64(SENTINEL)).all()
    return want


def go(lib, x, r, offs=(0, 0), peak=None):
    request, _, _ = frame(x, peak)
    st, words = run(lib, x, r, request, offs)
    assert st == 0, lib.kmp_last_error()
    assert lib.kmp_last_launch() == b'ssim'
    return check_words(words, x, r, request, peak)


def test_constants(kom):
    L = consts()
    assert (L.CODER_SSIM, L.SSIM_GROUPS, L.SSIM_BYTES) == (14, 1024, 64 * 1026)
    assert L.SSIM_TILE_H * L.SSIM_TILE_W == 256 and L.SSIM_TILE_D >= 1


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_images_and_volumes(kom, dtype):
    """Odd widths (13, 19: element reads), more than one tile and more than one item, pointers offset by one
    sample; a default and a caller's peak."""
    lib = kom._lib.lib
    for k, shape in enumerate(((3, 1, 13, 19), (2, 1, 40, 37), (2, 9, 13, 10), (2, 8, 19, 21))):
        x, r = field(shape, dtype, seed=10 + k)
        for offs in ((0, 0), (1, 1), (0, 1)):
            go(lib, x, r, offs)
        go(lib, x, r, peak=3.0 * S.default_frame(x)[0])


@pytest.mark.parametrize('dtype', [np.float32, np.uint8, np.uint16], ids=['float32', 'uint8', 'uint16'])
def test_every_extent_around_the_window_and_the_tile(kom, dtype):
    """Each spatial extent at 7 (one window), 8, tile + 5, tile + 6 (the tile's last full window) and tile + 7."""
    lib, L = kom._lib.lib, consts()
    seed = 100
    for axis, tile in ((1, L.SSIM_TILE_D), (2, L.SSIM_TILE_H), (3, L.SSIM_TILE_W)):
        for ext in (7, 8, tile + 5, tile + 6, tile + 7):
            shape = [2, 7, 8, 9]
            shape[axis] = ext
            seed += 1
            go(lib, *field(tuple(shape), dtype, seed))
            if axis != 1:  # images
                shape[1] = 1
                go(lib, *field(tuple(shape), dtype, seed))
    x, r = field((1, 7, 7, 7), dtype, 99)
    assert go(lib, x, r)['windows'] == 1
    x, r = field((1, 1, 7, 7), dtype, 98)
    assert go(lib, x, r)['windows'] == 1


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_widths_that_take_16_byte_reads(kom, dtype):
    """Aligned pointers and a width that is a multiple of 16 bytes: the chunked staging, one tile and several,
    a plane edge inside a chunk row; the same arrays one sample off take element reads."""
    lib = kom._lib.lib
    for k, shape in enumerate(((2, 1, 23, 16), (1, 1, 17, 48), (2, 8, 9, 32), (1, 39, 23, 64))):
        x, r = field(shape, dtype, seed=200 + k)
        a = go(lib, x, r)
        b = go(lib, x, r, offs=(1, 1))
        assert a['windows'] == b['windows']


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_items_do_not_leak(kom, dtype):
    """Three items at the bottom, the middle and the top of the range: a window straddling two items, or a
    halo read from the neighbour, moves the result far beyond the tolerance."""
    lib = kom._lib.lib
    for shape in ((3, 1, 9, 12), (3, 7, 8, 16), (3, 8, 23, 9)):
        x, r = field(shape, dtype, seed=31, levels=(0.0, 0.5, 1.0))
        go(lib, x, r)
        go(lib, x, r, offs=(1, 1))


def test_many_small_items_take_several_units_per_workgroup(kom):
    """More units than workgroups: 600 images of 7 x 7 (one window each, 115 workgroups) and 1100 volumes of
    7 x 7 x 7 (the grid is at its cap)."""
    lib, L = kom._lib.lib, consts()
    for dtype in (np.float32, np.uint8):
        x, r = field((600, 1, 7, 7), dtype, seed=41)
        assert L.ssim_groups(x.size) < 600
        assert go(lib, x, r)['windows'] == 600
        x, r = field((1100, 7, 7, 7), dtype, seed=42)
        assert L.ssim_groups(x.size) == L.SSIM_GROUPS < 1100
        assert go(lib, x, r)['windows'] == 1100


NONFINITE = (np.nan, np.inf, -np.inf)


@pytest.mark.parametrize('shape', [(2, 1, 12, 21), (2, 9, 10, 16)], ids=['2d', '3d'])
def test_float32_non_finite_values(kom, shape):
    lib = kom._lib.lib
    x0, r0 = field(shape, np.float32, seed=51)
    first, last = (0, 0, 0, 0), tuple(s - 1 for s in shape)
    inner = (1,) + tuple(s // 2 for s in shape[1:])
    for k, at in enumerate((first, last, (0,) + last[1:], (1, 0, 0, 0), inner)):
        for side in ('x', 'r', 'both'):
            x, r = x0.copy(), r0.copy()
            v = NONFINITE[k % 3]
            if side in ('x', 'both'):
                x[at] = v
            if side in ('r', 'both'):
                r[at] = NONFINITE[(k + 1) % 3] if side == 'both' else v
            want = go(lib, x, r, offs=(k % 2, k % 2))
            assert want['skipped'] >= 1
    # an item that is all NaN: its windows are skipped, the other item's counted; then every item
    x, r = x0.copy(), r0.copy()
    x[1] = np.nan
    want = go(lib, x, r)
    assert want['windows'] == want['skipped'] == S.windows_per_item(*shape[1:])
    r[0] = np.nan
    request = request_words(shape[1:], 1e-4, 9e-4, 0.0)
    st, words = run(lib, x, r, request)
    assert st == 0
    assert words[0] == 0 and words[1] == 2 * S.windows_per_item(*shape[1:]) and words[4] == 0
    assert words.view(np.float64)[2] == 0.0 and words.view(np.float64)[3] == math.inf


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_restored_equals_original(kom, dtype):
    """The spec gives exactly 1.0; the device may contract multiply-adds, so it is held to the tolerance."""
    lib = kom._lib.lib
    for shape in ((2, 1, 20, 24), (1, 9, 18, 13)):
        x, _ = field(shape, dtype, seed=61)
        want = go(lib, x, x.copy())
        assert want['ssim'] == 1.0 and want['min_ssim'] == 1.0


@pytest.mark.parametrize('dtype', [np.float32, np.uint16], ids=['float32', 'uint16'])
def test_two_calls_give_identical_buffers(kom, dtype):
    lib = kom._lib.lib
    for shape, offs in (((3, 1, 40, 50), (0, 0)), ((2, 40, 24, 40), (0, 0)), ((2, 9, 21, 19), (1, 1))):
        x, r = field(shape, dtype, seed=71)
        request, _, _ = frame(x)
        a = run(lib, x, r, request, offs)[1]
        b = run(lib, x, r, request, offs)[1]
        assert np.array_equal(a, b)
        check_words(a, x, r, request)


def test_a_graph_capture_replays_to_the_same_bits(kom):
    from kompressor_amd import _device as dev
    lib = kom._lib.lib
    x, r = field((2, 12, 20, 24), np.float32, seed=81)
    request, _, _ = frame(x)
    eager = run(lib, x, r, request)[1]
    xb, xp = G.placed(x, 0)
    rb, rp = G.placed(r, 0)
    out = fresh_out(request)

    def call():
        assert lib.kmp_code(0, SSIM, G.F32, rp, G.F32, xp, x.size, out.data_ptr(), dev.stream()) == 0
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for _ in range(2):
        out.copy_(fresh_out(request))
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint64), eager)


def test_malformed_requests_count_nothing(kom):
    """Ordinary argument checks the kernel reads from the request: status 1, zero counts, nothing else written."""
    lib, L = kom._lib.lib, consts()
    x, r = field((2, 8, 9, 10), np.float32, seed=91)
    good = dict(dims=(8, 9, 10), c1=1e-4, c2=9e-4, base=0.0)
    bad = [dict(good, dims=(8, 6, 15)), dict(good, dims=(3, 24, 10)), dict(good, dims=(8, 9, 11)), dict(good, dims=(8, 9, 0)),
           dict(good, dims=(0, 9, 10)), dict(good, dims=(-8, 9, 10)), dict(good, dims=(1 << 62, 1 << 62, 16)),
           dict(good, dims=(7, 7, 1 << 61)), dict(good, c2=0.0), dict(good, c1=math.nan), dict(good, c1=-1e-4),
           dict(good, c2=math.inf), dict(good, base=math.nan), dict(good, base=-math.inf)]
    groups = L.ssim_groups(x.size)
    for q in bad:
        request = request_words(q['dims'], q['c1'], q['c2'], q['base'])
        st, words = run(lib, x, r, request)
        assert st == 0, (q, lib.kmp_last_error())
        f = words.view(np.float64)
        assert words[0] == 0 and words[1] == 0 and f[2] == 0.0 and f[3] == math.inf and words[4] == 1, q
        assert (words[5:8] == 0).all() and np.array_equal(words[8:16].view(np.int64), request)
        part = words[16:16 + 8 * groups].reshape(groups, 8)
        assert (part[:, :2] == 0).all() and (part[:, 4] == 1).all() and (part[:, 5:] == 0).all()
        assert (words[16 + 8 * groups:] == np.uint64(SENTINEL)).all()
        with pytest.raises(ValueError):
            kom.metrics.ssim_summary(words[:8])
    request = request_words(**{k: good[k] for k in ('dims', 'c1', 'c2', 'base')})
    st, words = run(lib, x, r, request)
    assert st == 0 and words[4] == 0 and words[0] == 2 * S.windows_per_item(8, 9, 10)


def test_argument_errors(kom):
    from kompressor_amd import _device as dev
    lib = kom._lib.lib
    x = torch.zeros(7 * 7 * 8, dtype=torch.float32, device='cuda')
    r = torch.zeros(7 * 7 * 8, dtype=torch.float32, device='cuda')
    request = request_words((1, 7, 56), 1e-4, 9e-4, 0.0)
    out = fresh_out(request)
    n = x.numel()

    def code(direction, coder, pc, pred, xc, xx, count, o):
        return lib.kmp_code(direction, coder, pc, pred, xc, xx, count, o, dev.stream())

    def refused(status):
        assert status == KMP_ERR_ARG, (status, lib.kmp_last_error())

    X, R, O = x.data_ptr(), r.data_ptr(), out.data_ptr()
    F32, U8, U16, I32, U32, I8, I16 = G.F32, G.U8, G.U16, G.I32, G.U32, G.I8, G.I16
    assert code(0, SSIM, F32, R, F32, X, n, O) == 0
    torch.cuda.synchronize()
    first = out.cpu().numpy().view(np.uint64).copy()
    assert first[0] == 50 and first[4] == 0
    refused(code(0, SSIM, F32, None, F32, X, n, O))  # no restored array
    refused(code(0, SSIM, F32, None, F32, X, 0, O))  # ... before the count is looked at
    refused(code(1, SSIM, F32, R, F32, X, n, O))     # KMP_DECODE
    refused(code(2, SSIM, F32, R, F32, X, n, O))
    for field_ in (1, 2, 127, 255, 256, 1 << 20):
        refused(code(0, SSIM | (field_ << 8), F32, R, F32, X, n, O))  # a non-zero field
        refused(code(0, SSIM | (field_ << 8), F32, R, F32, X, 0, O))
    for xc, pc in ((F32, U8), (U8, F32), (U16, I16), (I8, U8), (I32, I32), (U32, U32), (99, 99), (-1, -1)):
        refused(code(0, SSIM, pc, R, xc, X, n, O))     # differing or unsupported dtypes
    for mis in (1, 2, 4, 7):
        refused(code(0, SSIM, F32, R, F32, X, n, O + mis))  # a misaligned out
    for mis in (1, 2, 3):
        refused(code(0, SSIM, F32, R + mis, F32, X, n - 1, O))  # arrays not aligned to their dtype
        refused(code(0, SSIM, F32, R, F32, X + mis, n - 1, O))
    refused(code(0, SSIM, U16, R + 1, U16, X, n, O))
    refused(code(0, SSIM, I16, R, I16, X + 1, n, O))
    refused(code(0, SSIM, F32, R, F32, X, -1, O))
    refused(code(0, SSIM, F32, R, F32, None, n, O))   # null pointers
    refused(code(0, SSIM, F32, R, F32, X, n, None))
    refused(code(0, -SSIM, F32, R, F32, X, n, O))
    # n == 0 is KMP_OK and touches nothing
    assert code(0, SSIM, F32, R, F32, None, 0, None) == 0
    assert code(0, SSIM, F32, R, F32, X, 0, O) == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint64), first)  # nothing was launched by a refusal


def test_other_entry_points_refuse_the_code(kom):
    """The fused codec and the callback path take no SSIM request: KMP_ERR_ARG, nothing launched."""
    from kompressor_amd import _lib, _nd
    lib = _lib.lib
    I16, F32 = G.I16, G.F32
    x = torch.zeros((1, 5, 5, 5, 1), dtype=torch.int16, device='cuda')
    lowres, maps, dims = _nd._alloc_encoded(x, _lib.CODER_U16, 3)
    probe = _lib.Predictor(0, 0, None, None)
    need = int(lib.kmp_volume_workspace_bytes(I16, 1, 5, 5, 5, 1, ctypes.byref(probe)))
    ws = torch.zeros((max(need, 8),), dtype=torch.uint8, device='cuda')
    dims_out = (ctypes.c_int32 * 3)()
    spare = [torch.zeros(256, dtype=torch.int16, device='cuda') for _ in range(7)]
    coder = _lib.CODER_SSIM
    st = [lib.kmp_volume_encode(I16, x.data_ptr(), 1, 5, 5, 5, 1, ctypes.byref(probe), coder, lowres.data_ptr(),
                                _lib.ptrs(maps), dims_out, None, ws.data_ptr(), need, None),
          lib.kmp_volume_decode(I16, lowres.data_ptr(), _lib.ptrs(maps), 1, *lowres.shape[1:4], 1,
                                _lib.i32xn(dims), ctypes.byref(probe), coder, x.data_ptr(), None, ws.data_ptr(),
                                need, None),
          lib.kmp_encode_with_predictions(3, I16, coder, x.data_ptr(), 1, _lib.i64x3((5, 5, 5)), 1, _lib.ptrs(spare),
                                          lowres.data_ptr(), _lib.ptrs(maps), None),
          lib.kmp_decode_with_predictions_typed(3, I16, coder, F32, lowres.data_ptr(), _lib.ptrs(maps), 1,
                                                _lib.i64x3(lowres.shape[1:4]), 1, _lib.i32xn(dims), _lib.ptrs(spare),
                                                x.data_ptr(), None)]
    assert st == [KMP_ERR_ARG] * 4, (st, lib.kmp_last_error())


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_metrics_ssim(kom, dtype):
    """numpy arrays and CUDA tensors in the package's layouts; channels are items, through a channel-first copy."""
    tol = S.TOL_F32 if dtype == np.float32 else S.TOL_INT
    for shape in ((2, 1, 11, 13), (1, 8, 9, 12)):
        for C in (1, 3):
            xs, rs = field((shape[0] * C,) + shape[1:], dtype, seed=5 + C, levels=np.linspace(0.2, 0.8, shape[0] * C))
            # (N, D, H, W) items -> (B, [D,] H, W, C)
            lay = lambda a: np.ascontiguousarray(np.moveaxis(  # noqa: E731
                a.reshape((shape[0], C) + (shape[2:] if shape[1] == 1 else shape[1:])), 1, -1))
            x, r = lay(xs), lay(rs)
            assert np.array_equal(S.items(x), xs)
            for peak in (None, 2.5 * S.default_frame(xs)[0]):
                want = S.ssim(xs, rs, peak)
                got = kom.metrics.ssim(x, r, peak)
                assert set(got) == {'ssim', 'min_ssim', 'windows', 'skipped', 'peak', 'base'}
                assert (got['windows'], got['skipped'], got['peak'], got['base']) == \
                    (want['windows'], want['skipped'], want['peak'], want['base'])
                assert abs(got['ssim'] - want['ssim']) <= tol and abs(got['min_ssim'] - want['min_ssim']) <= tol
                tx, tr = torch.from_numpy(x.copy()).cuda(), torch.from_numpy(r.copy()).cuda()
                assert kom.metrics.ssim(tx, tr, peak) == got and kom.metrics.ssim(x, tr, peak) == got
    if dtype == np.float32:
        flat = np.full((1, 9, 9, 1), 2.0, np.float32)
        with pytest.raises(ValueError):
            kom.metrics.ssim(flat, flat)  # no value range, no default peak
        assert kom.metrics.ssim(flat, flat, peak=1.0)['windows'] == 9
        nans = np.full((1, 9, 9, 1), np.nan, np.float32)
        got = kom.metrics.ssim(nans, flat, peak=1.0)
        assert got['windows'] == 0 and got['skipped'] == 9 and math.isnan(got['ssim'])
