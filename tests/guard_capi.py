"""One C-ABI launch under the guard-band harness, shared by the test_gpu_guard_* modules of the
non-fused entry points (primitives, callback path, packers and fit).

A launch is described by its tensors (:class:`T`): inputs filled with numpy data, outputs with the
oracle's expected value and an ownership mask, scratch (workspace).  :func:`launch` carves every one
of them from a sentinel-filled device arena of its own (guard_spec.py), at the pointer shifts of the
``shift`` mode, calls the entry point through ``kompressor_amd._lib.lib`` with the arena pointers,
twice (0xA5 and 0x5A arenas), and hands both runs to ``guard_spec.check_launch_pair``: guards, shift
bytes and inputs unchanged; unowned output elements still the sentinel; owned ones bit-equal to the
oracle; the two runs identical.

Shift modes (bytes per tensor; ``T.align`` is the alignment the header states for that pointer, else
one element of the tensor's own dtype):
  'none'  every pointer at its 256-byte aligned arena position;
  'all'   every tensor moved by one element (or by its stated alignment);
  'out'   inputs at 0, outputs and scratch moved;
  a dict  {tensor name: bytes} for a shift of single tensors.

``LAUNCHED`` collects (entry point, kmp_last_launch()) of every launch made, per calling module, so
each module's last test can assert that it reached what it declares in ``LAUNCHES``.
"""

import ctypes

import numpy as np
import pytest
import torch

import oracle
import guard_spec as G

NP2T = {np.dtype(np.uint8): torch.uint8, np.dtype(np.uint16): torch.uint16, np.dtype(np.int32): torch.int32,
        np.dtype(np.float32): torch.float32, np.dtype(np.uint32): torch.uint32, np.dtype(np.int64): torch.int64,
        np.dtype(np.uint64): torch.uint64}
CODE = {np.dtype(np.uint8): 0, np.dtype(np.uint16): 1, np.dtype(np.int32): 2, np.dtype(np.float32): 3,
        np.dtype(np.uint32): 4}
SHIFTS = ('none', 'all', 'out')

LAUNCHED = {}  # {entry point: set of kmp_last_launch() names}

# the sample dtypes, and the shapes whose row lengths lie around the 16-byte chunk boundaries
DTYPES = [np.uint8, np.uint16, np.int32, np.float32, np.uint32]
DT_IDS = [np.dtype(d).name for d in DTYPES]


def widths(dtype):
    V = 16 // np.dtype(dtype).itemsize
    return [3, 2 * V - 1, 2 * V, 2 * V + 1, 2 * V + 2, 4 * V + 1]


def shapes(dtype, nsp):
    """The C == 1 shapes of a dtype, then the one C == 3 shape (element kernels)."""
    out = []
    for i, w in enumerate(widths(dtype)):
        if nsp == 3:
            out.append((2, 5, 6, w, 1) if i % 2 == 0 else (2, 6, 5, w, 1))
        else:
            out.append((3, 7, w, 1) if i % 2 == 0 else (3, 8, w, 1))
    out.append((1, 5, 6, 7, 3) if nsp == 3 else (2, 7, 9, 3))
    return out


def ons(nsp):
    return oracle.volume if nsp == 3 else oracle.image


@pytest.fixture(params=['rows', 'elements'])
def form(request, kmp_opt):
    """Both kernels behind one launch name: the row form and (KMP_DISABLE_ROWS=1) the element form."""
    kmp_opt('KMP_DISABLE_ROWS', 1 if request.param == 'elements' else None)
    return request.param


class T:
    """One tensor of a launch.  ``role``: 'in' (``value`` = the data), 'out' (``value`` = the expected
    array; ``mask`` = owned elements, default all; ``judge`` = a predicate instead of bit equality, see
    check_launch_pair), 'scratch' (``value`` gives shape and dtype only), 'untouched' (as scratch, and
    the launch may not write it)."""

    def __init__(self, name, role, value, mask=None, align=None, judge=None):
        assert role in ('in', 'out', 'scratch', 'untouched')
        self.name, self.role, self.value = name, role, np.ascontiguousarray(value)
        self.mask, self.align, self.judge = mask, align, judge

    def shift_bytes(self, mode):
        step = self.align if self.align is not None else self.value.dtype.itemsize
        if isinstance(mode, dict):
            return int(mode.get(self.name, 0))
        if mode == 'all' or (mode == 'out' and self.role != 'in'):
            return step
        assert mode in SHIFTS
        return 0


def rand(shape, dtype, seed):
    """Full-range random samples (floats: normal, scaled past the 16-bit range)."""
    rng = np.random.default_rng(seed)
    dtype = np.dtype(dtype)
    if dtype == np.float32:
        return (rng.standard_normal(shape) * 3000).astype(np.float32)
    info = np.iinfo(dtype)
    return rng.integers(info.min, int(info.max) + 1, size=shape, dtype=np.int64).astype(dtype)


def i64x3(vals):
    vals = [int(v) for v in vals]
    return (ctypes.c_int64 * 3)(*(vals + [0] * (3 - len(vals))))


def i32x3(vals):
    vals = [int(v) for v in vals]
    return (ctypes.c_int32 * 3)(*(vals + [0] * (3 - len(vals))))


def ptr_array(ptrs, n=7):
    arr = (ctypes.c_void_p * n)()
    for i, p in enumerate(ptrs):
        arr[i] = p
    return arr


def launch(entry, tensors, call, shift='none', keep=None, prepare=None):
    """Runs ``call(lib_function, {name: device address})`` (returning the kmp_status) on arenas of
    ``tensors`` under check_launch_pair.  ``keep``: a list that receives each run's ``{name: Carved}``
    (for checks between two outputs of one launch, or of scratch the launch's contract describes);
    ``prepare({name: Carved})`` runs before the call (bytes the caller owes the launch inside a tensor
    the launch also writes).  Returns the launch's kmp_last_launch() name."""
    from kompressor_amd import _lib
    fn = getattr(_lib.lib, entry)
    names = []

    def run(sentinel):
        got = {}
        for t in tensors:
            c = G.carve_arena(t.value.shape, NP2T[t.value.dtype], 'cuda', sentinel, t.shift_bytes(shift))
            got[t.name] = G.fill(c, t.value) if t.role == 'in' else c
        ptrs = {n: c.arena.data_ptr() + G.GUARD + c.shift for n, c in got.items()}
        if prepare is not None:
            prepare(got)
        torch.cuda.synchronize()
        status = call(fn, ptrs)
        assert status == 0, f'{entry} returned {status}: {_lib.lib.kmp_last_error().decode(errors="replace")}'
        torch.cuda.synchronize()
        names.append(_lib.lib.kmp_last_launch().decode())
        if keep is not None:
            keep.append(got)
        return got

    outs = [t for t in tensors if t.role == 'out']
    G.check_launch_pair(
        run, {t.name: t.value for t in tensors if t.role == 'in'}, [t.name for t in outs],
        {t.name: t.value for t in outs if t.judge is None},
        {t.name: np.ones(t.value.shape, bool) if t.mask is None else t.mask for t in outs},
        untouched=tuple(t.name for t in tensors if t.role == 'untouched'),
        predicates={t.name: (t.value.dtype, t.judge) for t in outs if t.judge is not None})
    assert names[0] == names[1] and names[0], f'{entry}: launch names {names}'
    LAUNCHED.setdefault(entry, set()).add(names[0])
    return names[0]


def payload_numpy(carved):
    """The payload of a device arena as a numpy array of its dtype and shape (a copy)."""
    raw = carved.arena_bytes()[G.GUARD + carved.shift:G.GUARD + carved.shift + carved.nbytes].copy()
    np_dtype = {v: k for k, v in NP2T.items()}[carved.payload.dtype]
    return raw.view(np_dtype).reshape(tuple(carved.payload.shape))


def assert_declared_were_launched(declared):
    missing = [e for e in declared if not LAUNCHED.get(e)]
    assert not missing, f'declared in LAUNCHES but never launched by this run: {missing}'
