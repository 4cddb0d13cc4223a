"""Guard-band harness for the fused codec's launches, shared by test_guard_harness.py (the oracle
writing into CPU arenas) and test_gpu_guard.py (the kernels writing into device arenas).

Every tensor a launch touches is carved from an arena the test owns: ``GUARD`` bytes, an optional
pointer ``shift``, the payload, ``GUARD`` bytes, all filled with one sentinel byte.  A launch runs
twice, on ``0xA5`` and on ``0x5A`` arenas, and :func:`check_launch_pair` then reads every byte:
what the launch may not touch still holds the sentinel, what it owns holds the expected value in
both runs.  Pure torch / numpy; works on CPU and CUDA tensors alike; knows nothing of the product.

Ownership follows the C header's region contract ("a launch writes exactly the outputs whose block
coordinate lies in the box"): the box is the region clamped to the stored lowres extent ``[0, E)``
per axis; an encode owns the lowres nodes in the box and each map's entries in the box that exist
in that map's trimmed shape; a decode owns the highres samples whose block ``i // 2`` per axis
lies in the box.
"""

import numpy as np
import torch

GUARD = 4096  # bytes on either side: more than one wave's widest row store (64 lanes x 16 B)
ALIGN = 256   # payload alignment at shift 0
SENTINELS = (0xA5, 0x5A)


class GuardError(AssertionError):
    """``failures``: list of ``(check, tensor name, count)``; check is one of 'guard', 'input',
    'unowned', 'value', 'nondeterministic'."""

    def __init__(self, failures, lines):
        super().__init__('\n'.join(lines))
        self.failures = failures


class Carved:
    """One arena: ``arena`` (uint8, the whole of it), ``payload`` (the contiguous view a launch
    gets), ``shift`` (bytes between the leading guard and the payload)."""

    def __init__(self, arena, payload, shift, sentinel):
        self.arena, self.payload, self.shift, self.sentinel = arena, payload, shift, sentinel

    @property
    def nbytes(self):
        return self.payload.numel() * self.payload.element_size()

    def arena_bytes(self):
        """The arena as a numpy uint8 array (a copy for a device arena, a view on the CPU)."""
        a = self.arena
        return a.cpu().numpy() if a.is_cuda else a.numpy()


def _itemsize(dtype):
    return torch.empty(0, dtype=dtype).element_size()


def carve_arena(shape, dtype, device, sentinel, shift=0):
    shape = tuple(int(s) for s in shape)
    item = _itemsize(dtype)
    if shift < 0 or shift % item:
        raise ValueError(f'shift {shift} is not a multiple of the item size {item}')
    nbytes = int(np.prod(shape, dtype=np.int64)) * item
    total = GUARD + shift + nbytes + GUARD
    store = torch.empty(total + ALIGN, dtype=torch.uint8, device=device)
    pad = (-(store.data_ptr() + GUARD)) % ALIGN  # the payload of a shift-0 arena starts ALIGN-aligned
    arena = store[pad:pad + total]
    arena.fill_(sentinel)
    raw = arena[GUARD + shift:GUARD + shift + nbytes]
    assert raw.data_ptr() % ALIGN == shift % ALIGN and raw.data_ptr() % item == 0
    payload = raw.view(dtype).view(shape)
    assert payload.is_contiguous()
    # (torch gives an empty view no address)
    assert nbytes == 0 or payload.data_ptr() == arena.data_ptr() + GUARD + shift
    return Carved(arena, payload, shift, sentinel)


def carve(shape, dtype, device, sentinel, shift=0):
    """``(arena, payload)``: a uint8 arena laid out as GUARD bytes, ``shift`` bytes, the payload,
    GUARD bytes, every byte ``sentinel``; and the payload as a contiguous ``shape`` / ``dtype`` view."""
    c = carve_arena(shape, dtype, device, sentinel, shift)
    return c.arena, c.payload


def fill(carved, values):
    """Copies the numpy array ``values`` (same shape and item size) into the payload, bytewise."""
    values = np.ascontiguousarray(values)
    assert values.nbytes == carved.nbytes and tuple(values.shape) == tuple(carved.payload.shape)
    src = torch.from_numpy(values.reshape(-1).view(np.uint8))
    a = carved.arena
    a[GUARD + carved.shift:GUARD + carved.shift + carved.nbytes].copy_(src)
    return carved


# ---------------------------------------------------------------------------------------------
# Ownership masks
# ---------------------------------------------------------------------------------------------

def clamp_box(region, E):
    """The region clamped per axis to ``[0, E)`` as ``[(begin, end), ...]``; ``None`` = the whole
    frame; an axis with ``end <= begin`` comes out as ``(0, 0)`` (an empty box)."""
    if region is None:
        return [(0, int(e)) for e in E]
    assert len(region) == len(E)
    box = []
    for (b, e), ext in zip(region, E):
        b, e = max(int(b), 0), min(int(e), int(ext))
        box.append((b, e) if e > b else (0, 0))
    return box


def _box_mask(shape, box, nsp):
    """True over ``[:, box..., ...]`` (spatial axes 1..nsp) clipped to ``shape``."""
    m = np.zeros(tuple(int(s) for s in shape), dtype=bool)
    m[(slice(None), *[slice(b, min(e, int(s))) for (b, e), s in zip(box, shape[1:1 + nsp])])] = True
    return m


def copy_box_mask(shape, offsets, extents, nsp):
    """True over ``[:, o:o + e per spatial axis, ...]``: what a box copy into an array of ``shape`` owns."""
    return _box_mask(shape, [(int(o), int(o) + int(e)) for o, e in zip(offsets, extents)], nsp)


def encode_masks(lowres_shape, map_shapes, region, nsp):
    """``{'lowres': mask, 'map0': mask, ...}`` for an encode launch with ``region``.  ``map_shapes``
    are the trimmed map shapes (the oracle's outputs): a map entry is owned iff its coordinate is in
    the box, which the map's own (possibly one shorter) extent clips."""
    box = clamp_box(region, lowres_shape[1:1 + nsp])
    masks = {'lowres': _box_mask(lowres_shape, box, nsp)}
    for k, s in enumerate(map_shapes):
        masks[f'map{k}'] = _box_mask(s, box, nsp)
    return masks


def decode_masks(highres_shape, lowres_shape, region, nsp):
    """``{'highres': mask}`` for a decode launch: sample ``i`` on an axis belongs to block ``i // 2``."""
    box = clamp_box(region, lowres_shape[1:1 + nsp])
    m = np.ones(tuple(int(s) for s in highres_shape), dtype=bool)
    for a, (b, e) in enumerate(box):
        n = int(highres_shape[1 + a])
        blk = np.arange(n) // 2
        keep = (blk >= b) & (blk < e)
        m &= keep.reshape([n if ax == 1 + a else 1 for ax in range(m.ndim)])
    return {'highres': m}


# ---------------------------------------------------------------------------------------------
# The checker
# ---------------------------------------------------------------------------------------------

def _first(idx, n=3):
    return [int(i) for i in idx[:n]]


def _elem_report(bad, shape, item):
    flat = np.flatnonzero(bad)
    where = [(tuple(int(v) for v in np.unravel_index(i, shape)), int(i) * item) for i in flat[:3]]
    return int(flat.size), ', '.join(f'{ix} at byte {off:+d}' for ix, off in where)


def _split(c):
    """(bytes before the payload, payload bytes, bytes after) of a carved arena, as numpy uint8."""
    a = c.arena_bytes()
    lo = GUARD + c.shift
    return a[:lo], a[lo:lo + c.nbytes], a[lo + c.nbytes:]


def check_launch_pair(run, inputs, outputs, expected, masks, untouched=(), predicates=None):
    """``run(sentinel)`` performs one launch on arenas filled with ``sentinel`` and returns
    ``{name: Carved}`` of EVERY tensor the launch was given (inputs, outputs, workspace).
    ``inputs``: ``{name: numpy array}`` the input payloads were filled with; ``outputs``: names of
    the tensors the launch writes; ``expected``: ``{name: numpy array}`` per output; ``masks``:
    ``{name: bool array}``, the elements the launch owns.  Tensors named in neither ``inputs`` nor
    ``outputs`` (the workspace) are scratch: only their guards are checked, unless they are named
    in ``untouched`` (a launch that must write nothing at all: the payload still the sentinel).
    ``predicates``: ``{name: (numpy dtype, wrong)}`` for an output whose owned values are not pinned
    bit for bit: ``wrong(values)`` gets the payload as an array of that dtype and the tensor's shape
    and returns the bool array of elements that miss the output's bound; it replaces the bytewise
    comparison of check c for that output (``expected`` needs no entry for it), nothing else.

    Raises :class:`GuardError` listing every violation of
      a. guard, shift and input bytes unchanged;
      b. unowned output elements still the sentinel, in both runs;
      c. owned output elements equal to ``expected``, in both runs;
      d. the two runs' owned bytes identical."""
    failures, lines = [], []

    def fail(check, name, count, text):
        failures.append((check, name, count))
        lines.append(f'[{check}] {name}: {count} {text}')

    owned_bytes = []
    for sentinel in SENTINELS:
        got = run(sentinel)
        assert set(inputs) <= set(got) and set(outputs) <= set(got), 'run() must return every tensor it used'
        tag = f'(sentinel 0x{sentinel:02X})'
        owned = {}
        for name, c in got.items():
            assert c.sentinel == sentinel, f'{name} was not carved with this run\'s sentinel'
            pre, body, post = _split(c)
            # a. guards and shift bytes (offsets relative to the payload: negative = before it)
            bad = np.concatenate([np.flatnonzero(pre != sentinel) - pre.size,
                                  np.flatnonzero(post != sentinel) + c.nbytes])
            if bad.size:
                fail('guard', name, int(bad.size), f'guard bytes changed {tag}, first at payload offset '
                     + ', '.join(f'{o:+d}' for o in _first(bad)))
            shape = tuple(c.payload.shape)
            item = c.payload.element_size()
            if name in inputs:
                want = np.ascontiguousarray(inputs[name]).reshape(-1).view(np.uint8)
                assert want.size == body.size, f'{name}: input reference has another size'
                diff = (body != want).reshape(-1, item).any(axis=1)
                if diff.any():
                    n, txt = _elem_report(diff, shape, item)
                    fail('input', name, n, f'input elements modified {tag}: {txt}')
                continue
            if name not in outputs:
                if name in untouched:
                    bad = np.flatnonzero(body != sentinel)
                    if bad.size:
                        fail('unowned', name, int(bad.size), f'bytes written by a launch that owns nothing {tag}, '
                             'first at payload offset ' + ', '.join(f'{o:+d}' for o in _first(bad)))
                continue
            elems = body.reshape(-1, item)
            mask = np.asarray(masks[name], dtype=bool)
            assert mask.shape == shape, f'{name}: mask shape {mask.shape} != tensor shape {shape}'
            mflat = mask.reshape(-1)
            # b. everything outside the ownership mask still holds the sentinel
            stray = ~mflat & (elems != sentinel).any(axis=1)
            if stray.any():
                n, txt = _elem_report(stray, shape, item)
                fail('unowned', name, n, f'elements written outside the launch\'s box {tag}: {txt}')
            # c. everything inside equals the reference (or meets the caller's bound)
            if predicates and name in predicates:
                pdtype, judge = predicates[name]
                assert np.dtype(pdtype).itemsize == item, f'{name}: predicate dtype {pdtype} is not {item} B'
                miss = np.asarray(judge(body.copy().view(pdtype).reshape(shape)), dtype=bool)
                assert miss.shape == shape, f'{name}: predicate returned shape {miss.shape}, tensor is {shape}'
                wrong = mflat & miss.reshape(-1)
            else:
                want = np.ascontiguousarray(expected[name])
                assert tuple(want.shape) == shape and want.dtype.itemsize == item, \
                    f'{name}: expected {want.shape} {want.dtype}, tensor is {shape} x {item} B'
                wrong = mflat & (elems != want.reshape(-1).view(np.uint8).reshape(-1, item)).any(axis=1)
            if wrong.any():
                n, txt = _elem_report(wrong, shape, item)
                fail('value', name, n, f'owned elements differ from the reference {tag}: {txt}')
            owned[name] = (elems[mflat].copy(), np.flatnonzero(mflat), shape, item)
        owned_bytes.append(owned)
    # d. run-to-run: the owned bytes must not depend on the surroundings or on workspace contents
    for name, (e0, idx, shape, item) in owned_bytes[0].items():
        e1 = owned_bytes[1][name][0]
        diff = (e0 != e1).any(axis=1)
        if diff.any():
            bad = np.zeros(int(np.prod(shape, dtype=np.int64)), dtype=bool)
            bad[idx[diff]] = True
            n, txt = _elem_report(bad, shape, item)
            fail('nondeterministic', name, n, f'owned elements differ between the two runs: {txt}')
    if failures:
        raise GuardError(failures, lines)
