"""The kernels of masked float32 fields on the GPU: kmp_code with KMP_CODER_FILL and
KMP_CODER_RUNS against tests/runs_spec.py, bit for bit -- the counts around a wave, a workgroup step and a
workgroup's span, the carries across whole workgroups, both access forms, determinism, every KMP_ERR_ARG
case with nothing launched -- and ``kom.quant``'s functions over them on numpy and CUDA inputs."""

import numpy as np
import pytest
import torch

import quant_spec as Q
import runs_spec as R

pytestmark = pytest.mark.gpu

KMP_ERR_ARG = -1
U8, U16, I32, F32, U32, I8, I16 = 0, 1, 2, 3, 4, 5, 6
CODE = {np.dtype(np.int16): I16, np.dtype(np.int32): I32}
FILL, RUNS = 11, 12
TILE, FILL_BYTES, PIECE = 2048, 16384, 256
# a workgroup's span is ceil(ceil(n / TILE) / 1024) * TILE elements (``_lib.fill_span``): one tile up to
# 1024 * TILE elements, so three workgroups run from 2 * TILE + 1 elements on
THREE = 2 * TILE + 1
SENTINEL = 0x5A
DTYPES = [np.int16, np.int32]
IDS = ['int16', 'int32']
NAN, NAN2, PINF = 0x7fc00000, 0x7fc00001, 0x7f800000


def placed(a, off_bytes=0, pad=64):
    """``a``'s bytes on the device ``off_bytes`` past a 256-byte boundary, sentinel bytes around them:
    (buffer, address)."""
    a = np.ascontiguousarray(a)
    buf = torch.full((a.nbytes + 2 * pad + 256,), SENTINEL, dtype=torch.uint8, device='cuda')
    assert buf.data_ptr() % 256 == 0
    lo = 256 + off_bytes
    if a.nbytes:
        buf[lo:lo + a.nbytes] = torch.from_numpy(a.reshape(-1).view(np.uint8)).cuda()
    return buf, buf.data_ptr() + lo


def payload(buf, off_bytes, like):
    lo = 256 + off_bytes
    return buf[lo:lo + like.nbytes].cpu().numpy().view(like.dtype).reshape(like.shape)


def untouched_around(buf, off_bytes, nbytes):
    b = buf.cpu().numpy()
    lo = 256 + off_bytes
    return (b[:lo] == SENTINEL).all() and (b[lo + nbytes:] == SENTINEL).all()


def fill_call(lib, marked, xoff=0, ooff=0, inplace=False):
    """One FILL call on fresh buffers: (status, result array, everything around the output untouched)."""
    from kompressor_amd import _device as dev
    xb, xp = placed(marked, xoff)
    ob, op = (xb, xp) if inplace else placed(np.zeros_like(marked), ooff)
    if not inplace:
        ob[256 + ooff:256 + ooff + marked.nbytes] = SENTINEL
    ws = torch.full((FILL_BYTES,), SENTINEL, dtype=torch.uint8, device='cuda')
    st = lib.kmp_code(0, FILL, 0, ws.data_ptr(), CODE[marked.dtype], xp, marked.size, op, dev.stream())
    torch.cuda.synchronize()
    off = xoff if inplace else ooff
    same_in = inplace or np.array_equal(payload(xb, xoff, marked), marked)
    return st, payload(ob, off, marked), untouched_around(ob, off, marked.nbytes) and same_in


def random_marked(n, dtype, seed, p=0.3):
    """Full-range values, a fraction ``p`` of them marked in stretches of random length."""
    rng = np.random.default_rng(seed)
    info = np.iinfo(dtype)
    x = rng.integers(info.min + 1, int(info.max) + 1, size=n, dtype=np.int64).astype(dtype)
    at = 0
    while at < n:
        length = int(rng.integers(1, 200))
        if rng.random() < p:
            x[at:at + length] = info.min
        at += length
    return x


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_fill_counts(kom, dtype):
    lib = kom._lib.lib
    # around a wave, a workgroup (one item of 8 per lane: 512 and 2048 elements), a count that is no
    # multiple of the 8-element item, and the span boundaries
    for n in (1, 7, 8, 9, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1003, TILE - 1, TILE, TILE + 1, THREE):
        for seed, p in ((n, 0.3), (n + 1, 0.9)):
            marked = random_marked(n, dtype, seed, p)
            st, got, clean = fill_call(lib, marked)
            assert st == 0 and clean and np.array_equal(got, R.fill(marked)), (n, p)
    assert lib.kmp_last_launch().decode() == 'fill'


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('case', ['middle span marked', 'first span marked', 'first two spans marked',
                                  'all marked', 'none marked', 'only the last unmarked', 'only the first unmarked'])
def test_fill_carries_across_workgroups(kom, dtype, case):
    from kompressor_amd import _lib
    assert _lib.fill_span(THREE) == TILE and -(-THREE // TILE) == 3  # three workgroups, the third of one element
    M = R.mark(dtype)
    x = random_marked(THREE, dtype, 11, 0.0)
    if case == 'middle span marked':
        x[TILE:2 * TILE] = M
    elif case == 'first span marked':
        x[:TILE] = M
    elif case == 'first two spans marked':
        x[:2 * TILE] = M
    elif case == 'all marked':
        x[:] = M
    elif case == 'only the last unmarked':
        x[:-1] = M
    elif case == 'only the first unmarked':
        x[1:] = M
    for inplace in (False, True):
        st, got, clean = fill_call(_lib.lib, x, inplace=inplace)
        assert st == 0 and clean and np.array_equal(got, R.fill(x)), inplace


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_fill_many_tiles_per_workgroup(kom, dtype):
    """More tiles than workgroups: a span of two tiles, the running carry between a workgroup's steps."""
    from kompressor_amd import _lib
    n = 1024 * TILE + 5
    assert _lib.fill_span(n) == 2 * TILE
    x = random_marked(n, dtype, 5, 0.5)
    x[3 * TILE - 10:7 * TILE + 3] = R.mark(dtype)  # across steps and spans
    xt = torch.from_numpy(x).cuda()
    got = kom.quant.d_fill(xt)
    assert np.array_equal(got.cpu().numpy(), R.fill(x))
    assert np.array_equal(xt.cpu().numpy(), x)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_fill_element_form_and_determinism(kom, dtype):
    lib = kom._lib.lib
    w = np.dtype(dtype).itemsize
    for n in (1, 65, 1003, THREE):
        marked = random_marked(n, dtype, n + 7, 0.4)
        want = R.fill(marked)
        for xoff, ooff in ((w, w), (w, 0), (0, w), (8, 0), (0, 0)):
            a = fill_call(lib, marked, xoff, ooff)
            b = fill_call(lib, marked, xoff, ooff)
            assert a[0] == 0 and a[2] and np.array_equal(a[1], want), (n, xoff, ooff)
            assert b[0] == 0 and a[1].tobytes() == b[1].tobytes()
    # two calls on the very same buffers
    from kompressor_amd import _device as dev
    marked = random_marked(THREE, dtype, 3, 0.5)
    xb, xp = placed(marked)
    ob, op = placed(np.zeros_like(marked))
    ws = torch.zeros((FILL_BYTES,), dtype=torch.uint8, device='cuda')
    outs = []
    for _ in range(2):
        assert lib.kmp_code(0, FILL, 0, ws.data_ptr(), CODE[marked.dtype], xp, marked.size, op, dev.stream()) == 0
        torch.cuda.synchronize()
        outs.append((ob.cpu().numpy().tobytes(), ws.cpu().numpy().tobytes()))
    assert outs[0] == outs[1]


def table_of(starts, lengths, bits):
    t = np.zeros((len(starts), 4), np.uint32)
    s = np.asarray(starts, np.int64)
    t[:, 0], t[:, 1] = s & 0xffffffff, s >> 32
    t[:, 2], t[:, 3] = lengths, bits
    return t


def runs_call(lib, table, out, ooff=0, n=None):
    from kompressor_amd import _device as dev
    tb, tp = placed(table)
    ob, op = placed(out, ooff)
    st = lib.kmp_code(1, RUNS, 0, None, U32, tp, table.shape[0] if n is None else n, op, dev.stream())
    torch.cuda.synchronize()
    return st, payload(ob, ooff, out), untouched_around(ob, ooff, out.nbytes)


def patched(out, table):
    want = out.copy().view(np.uint32)
    for lo, hi, length, bits in table.tolist():
        want[(hi << 32 | lo):(hi << 32 | lo) + length] = bits
    return want.view(np.float32)


RUN_CASES = {
    'lengths 1, 63, 64, 65': ([3, 10, 100, 200], [1, 63, 64, 65], [NAN, PINF, NAN2, 0xff800000]),
    'short and long around the lane limit': ([0, 20, 40, 60, 80], [7, 8, 9, 10, 2], [1, 2, 3, 4, 5]),
    'a piece and one element': ([5], [PIECE + 1], [NAN]),
    'adjacent, different bits': ([50, 58, 70, 71], [8, 12, 1, 1], [NAN, PINF, NAN2, NAN]),
    'at index 0 and ending at numel': ([0, 40000 - 33], [17, 33], [NAN, PINF]),
    'one run over everything': ([0], [40000], [NAN2]),
    'more than 64 long runs': (list(range(0, 39000, 300)), [100 + i % 50 for i in range(130)], list(range(130))),
}


@pytest.mark.parametrize('case', list(RUN_CASES))
def test_runs(kom, case):
    lib = kom._lib.lib
    table = table_of(*RUN_CASES[case])
    out = np.random.default_rng(1).standard_normal(40000).astype(np.float32)
    for ooff in (0, 4, 8, 12):
        st, got, clean = runs_call(lib, table, out, ooff)
        assert st == 0 and clean and np.array_equal(got.view(np.uint32), patched(out, table).view(np.uint32)), ooff
    assert lib.kmp_last_launch().decode() == 'runs'


def test_runs_thousand_single_elements_and_none(kom):
    lib = kom._lib.lib
    rng = np.random.default_rng(2)
    starts = np.sort(rng.choice(5000, 1000, replace=False))
    table = table_of(starts, np.ones(1000, np.int64), rng.integers(0, 2 ** 32, size=1000, dtype=np.uint64))
    out = rng.standard_normal(5000).astype(np.float32)
    st, got, clean = runs_call(lib, table, out)
    assert st == 0 and clean and np.array_equal(got.view(np.uint32), patched(out, table).view(np.uint32))
    st, got, clean = runs_call(lib, table, out, n=0)  # R == 0
    assert st == 0 and clean and np.array_equal(got.view(np.uint32), out.view(np.uint32))


def test_argument_errors(kom):
    from kompressor_amd import _device as dev
    lib = kom._lib.lib
    x = torch.full((64,), -7, dtype=torch.int32, device='cuda')
    out = torch.full((64,), 0x5A5A5A5A, dtype=torch.int32, device='cuda')
    ws = torch.full((FILL_BYTES + 64,), SENTINEL, dtype=torch.uint8, device='cuda')
    table = torch.from_numpy(table_of([0], [4], [NAN]).view(np.int32)).cuda()
    f = torch.full((64,), 0x5A5A5A5A, dtype=torch.int32, device='cuda')

    def code(direction, coder, pc, pred, xc, xx, n, o):
        return lib.kmp_code(direction, coder, pc, pred, xc, xx, n, o, dev.stream())

    def refused(status):
        assert status == KMP_ERR_ARG, (status, lib.kmp_last_error())

    X, O, W, TB, FP = x.data_ptr(), out.data_ptr(), ws.data_ptr(), table.data_ptr(), f.data_ptr()
    # ---- FILL
    refused(code(1, FILL, 0, W, I32, X, 8, O))  # KMP_DECODE
    refused(code(2, FILL, 0, W, I32, X, 8, O))
    for xc in (U8, U16, F32, U32, I8, 99, -1):
        refused(code(0, FILL, 0, W, xc, X, 8, O))  # another dtype
    for field in (1, 2, 255, 1 << 20):
        refused(code(0, FILL | (field << 8), 0, W, I32, X, 8, O))
        refused(code(0, FILL | (field << 8), 0, W, I32, X, 0, O))
    refused(code(0, FILL, 0, None, I32, X, 8, O))  # no scratch
    refused(code(0, FILL, 0, None, I32, X, 0, O))  # ... before the count is looked at
    for mis in (1, 2, 4, 7):
        refused(code(0, FILL, 0, W + mis, I32, X, 8, O))  # a misaligned scratch
    for mis in (1, 2, 3):
        refused(code(0, FILL, 0, W, I32, X + mis, 8, O))  # arrays off their dtype's alignment
        refused(code(0, FILL, 0, W, I32, X, 8, O + mis))
    refused(code(0, FILL, 0, W, I16, X + 1, 8, O))
    refused(code(0, FILL, 0, W, I32, X, 8, X + 4))  # overlapping in part
    refused(code(0, FILL, 0, W, I32, X + 16, 8, X))
    refused(code(0, FILL, 0, W, I32, X, -1, O))
    refused(code(0, FILL, 0, W, I32, None, 8, O))
    refused(code(0, FILL, 0, W, I32, X, 8, None))
    assert code(0, FILL, 0, W, I32, None, 0, None) == 0  # nothing to do
    # ---- RUNS
    refused(code(0, RUNS, 0, None, U32, TB, 1, FP))  # KMP_ENCODE
    refused(code(2, RUNS, 0, None, U32, TB, 1, FP))
    for xc in (U8, U16, I32, F32, I8, I16, 99, -1):
        refused(code(1, RUNS, 0, None, xc, TB, 1, FP))
    for field in (1, 255, 1 << 20):
        refused(code(1, RUNS | (field << 8), 0, None, U32, TB, 1, FP))
        refused(code(1, RUNS | (field << 8), 0, None, U32, TB, 0, FP))
    refused(code(1, RUNS, 0, W, U32, TB, 1, FP))  # a prediction
    refused(code(1, RUNS, 0, W, U32, TB, 0, FP))
    for mis in (1, 4, 8):
        refused(code(1, RUNS, 0, None, U32, TB + mis, 1, FP))  # a misaligned table
    for mis in (1, 2, 3):
        refused(code(1, RUNS, 0, None, U32, TB, 1, FP + mis))  # a misaligned array
    refused(code(1, RUNS, 0, None, U32, TB, -1, FP))
    refused(code(1, RUNS, 0, None, U32, None, 1, FP))
    refused(code(1, RUNS, 0, None, U32, TB, 1, None))
    assert code(1, RUNS, 0, None, U32, None, 0, None) == 0
    refused(code(0, 13, 0, W, I32, X, 8, O))  # the next code is nobody's
    torch.cuda.synchronize()
    # nothing was launched by a refusal
    assert (out.cpu().numpy() == 0x5A5A5A5A).all() and (f.cpu().numpy() == 0x5A5A5A5A).all()
    assert (ws.cpu().numpy() == SENTINEL).all() and (x.cpu().numpy() == -7).all()


def test_other_entry_points_refuse_the_codes(kom):
    """The fused codec and the callback path take neither code: KMP_ERR_ARG, nothing launched."""
    import ctypes
    from kompressor_amd import _lib, _nd
    lib = _lib.lib
    x = torch.full((1, 5, 5, 5, 1), 77, dtype=torch.int16, device='cuda')
    lowres, maps, dims = _nd._alloc_encoded(x, _lib.CODER_U16, 3)
    probe = _lib.Predictor(0, 0, None, None)
    need = int(lib.kmp_volume_workspace_bytes(I16, 1, 5, 5, 5, 1, ctypes.byref(probe)))
    ws = torch.zeros((max(need, 8),), dtype=torch.uint8, device='cuda')
    dims_out = (ctypes.c_int32 * 3)()
    img = torch.full((1, 5, 5, 1), 77, dtype=torch.int16, device='cuda')
    ilow, imaps, idims = _nd._alloc_encoded(img, _lib.CODER_U16, 2)
    probe2 = _lib.Predictor(0, 0, None, None)
    spare = [torch.zeros(256, dtype=torch.int16, device='cuda') for _ in range(7)]
    outs = [lowres, *maps, ilow, *imaps]
    for t in outs:
        t.view(torch.uint8).fill_(SENTINEL)
    for coder in (_lib.CODER_FILL, _lib.CODER_RUNS, _lib.CODER_FILL | (1 << 8), _lib.CODER_RUNS | (3 << 8)):
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
    torch.cuda.synchronize()
    assert all((t.view(torch.uint8) == SENTINEL).all().item() for t in outs)  # no encode wrote anything
    assert (x == 77).all().item() and (img == 77).all().item()  # and no decode


# ---- kom.quant ------------------------------------------------------------------------------------------

def exceptions_case(seed=0):
    rng = np.random.default_rng(seed)
    idx = np.unique(np.concatenate([np.arange(100, 400), np.arange(400, 420), rng.choice(30000, 200, replace=False),
                                    [0, 29999]])).astype(np.int64)
    bits = np.full(idx.size, NAN, np.uint32)
    bits[(idx >= 400) & (idx < 420)] = PINF
    bits[::7] = NAN2
    return idx, bits


def test_quant_runs_round_trip(kom):
    q = kom.quant
    idx, bits = exceptions_case()
    want = R.runs((idx, bits))
    got = q.runs((idx, bits))
    assert all(isinstance(a, np.ndarray) and a.dtype == np.uint32 for a in got)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    back = q.exceptions_from_runs(*got)
    assert back[0].dtype == np.int64 and np.array_equal(back[0], idx) and np.array_equal(back[1], bits)
    # CUDA tensors in, CUDA tensors out
    tg = q.runs((torch.from_numpy(idx).cuda(), torch.from_numpy(bits).cuda()))
    assert all(t.is_cuda and t.dtype == torch.uint32 for t in tg)
    assert all(np.array_equal(t.cpu().numpy(), b) for t, b in zip(tg, want))
    tb = q.exceptions_from_runs(*tg)
    assert tb[0].is_cuda and np.array_equal(tb[0].cpu().numpy(), idx) and np.array_equal(tb[1].cpu().numpy(), bits)
    # indices above 2**32 and the empty list
    big = (np.array([1, 2 ** 32 + 5, 2 ** 32 + 6, 2 ** 40], np.int64), np.array([NAN, PINF, PINF, 7], np.uint32))
    assert all(np.array_equal(a, b) for a, b in zip(q.runs(big), R.runs(big)))
    none = (np.zeros(0, np.int64), np.zeros(0, np.uint32))
    assert all(a.shape == (0,) for a in q.runs(none))
    with pytest.raises(ValueError):
        q.exceptions_from_runs(*[np.zeros(2, np.uint32)] * 4)  # runs of length 0


def test_quant_table_cuts_long_runs_and_checks_extents(kom):
    q = kom.quant
    idx = np.concatenate([np.arange(10, 10 + 2 * PIECE + 1), [99990]]).astype(np.int64)
    bits = np.full(idx.size, NAN, np.uint32)
    bits[-1] = PINF
    stored = [torch.from_numpy(a).cuda() for a in R.runs((idx, bits))]
    table = q.d_run_table(*stored, 100000).cpu().numpy()
    assert table.tolist() == [[10, 0, PIECE, NAN], [10 + PIECE, 0, PIECE, NAN], [10 + 2 * PIECE, 0, 1, NAN],
                              [99990, 0, 1, PINF]]
    out = torch.zeros(100000, dtype=torch.float32, device='cuda')
    q.d_patch_runs(out, q.d_run_table(*stored, 100000))
    want = np.zeros(100000, np.uint32)
    want[idx] = bits
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want)
    with pytest.raises(ValueError):
        q.d_run_table(*stored, 99990)  # the last run ends past the array
    bad = [a.copy() for a in R.runs((idx, bits))]
    bad[2][0] = 0
    bad = [torch.from_numpy(a).cuda() for a in bad]
    with pytest.raises(ValueError):
        q.d_run_table(*bad, 100000)  # an empty run


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_quant_fill(kom, dtype):
    q = kom.quant
    idx, bits = exceptions_case(1)
    n = np.random.default_rng(4).integers(-3000, 3000, size=30000).astype(dtype).reshape(30, 1000)
    n.reshape(-1)[idx] = 0
    want = R.fill(R.marked(n, (idx, bits)))
    got = q.fill(n, (idx, bits))
    assert isinstance(got, np.ndarray) and got.dtype == n.dtype and np.array_equal(got, want)
    tg = q.fill(torch.from_numpy(n).cuda(), (torch.from_numpy(idx).cuda(), torch.from_numpy(bits).cuda()))
    assert tg.is_cuda and np.array_equal(tg.cpu().numpy(), want)
    assert np.array_equal(q.fill(n, None), n)
    with pytest.raises(ValueError):
        q.fill(n, (np.array([30000], np.int64), np.array([1], np.uint32)))


def test_quantise_is_unchanged_and_restores_the_same(kom):
    q = kom.quant
    x = Q.spec_field()[:, :10].copy()
    x[0, 2:4] = np.nan
    x[0, 7, 5, 5:9] = np.inf
    n, exc = q.quantise(x, 2.0 ** -7)
    ns, es = Q.quantise(x, -6)
    assert np.array_equal(n, ns) and np.array_equal(exc[0], es[0]) and np.array_equal(exc[1], es[1])  # 0 at exceptions
    filled = q.fill(n, exc)
    assert np.array_equal(filled, R.fill(R.marked(ns, es)))
    a, b = q.restore(n, -6, exc), q.restore(filled, -6, exc)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
