"""The guard-band harness (guard_spec.py) can fail: the oracle, writing into CPU arenas exactly the
elements a region launch owns, passes; every deliberately wrong writer is flagged with the right
tensor named; the ownership masks of z / row slabs that tile the frame partition every tensor."""

import functools

import numpy as np
import pytest
import torch

import oracle
from oracle import predictors as OP
import guard_spec as G

NP2T = {np.dtype(np.uint8): torch.uint8, np.dtype(np.uint16): torch.uint16, np.dtype(np.int32): torch.int32}
WS_BYTES = 64


@functools.lru_cache(maxsize=None)
def _reference(ndim):
    """x, the oracle's encode of it and the decode of that (MeanPredictor p = 1)."""
    if ndim == 3:
        ns, shape, dtype = oracle.volume, (2, 9, 14, 32, 1), np.uint16
        enc, dec = ns.encode_values_uint16, ns.decode_values_uint16
    else:
        ns, shape, dtype = oracle.image, (2, 31, 48, 1), np.uint8
        enc, dec = ns.encode_values_uint8, ns.decode_values_uint8
    x = np.random.default_rng(5).integers(0, np.iinfo(dtype).max + 1, size=shape).astype(dtype)
    fn = OP.mean_predictions_fn(1, ndim)
    lo, (maps, dims) = ns.encode(fn, enc, x, padding=1)
    maps = [np.ascontiguousarray(m) for m in maps]
    back = ns.decode(fn, dec, lo, (maps, dims), padding=1)
    assert np.array_equal(back, x)
    return x, np.ascontiguousarray(lo), maps, tuple(dims), back


def _region(ndim, span):
    """A z (volume) / row (image) span as a full region."""
    if span is None:
        return None
    lo = _reference(ndim)[1]
    return [span] + [(0, int(e)) for e in lo.shape[2:1 + ndim]]


def _carve_np(arr, sentinel, filled):
    c = G.carve_arena(arr.shape, NP2T[arr.dtype], 'cpu', sentinel)
    return G.fill(c, arr) if filled else c


def encode_launch(ndim, span, mutate=None):
    """(run, inputs, outputs, expected, masks) of the oracle as an encode 'kernel' with a region."""
    x, lo, maps, _, _ = _reference(ndim)
    expected = {'lowres': lo, **{f'map{k}': m for k, m in enumerate(maps)}}
    masks = G.encode_masks(lo.shape, [m.shape for m in maps], _region(ndim, span), ndim)

    def run(sentinel):
        t = {'highres': _carve_np(x, sentinel, True),
             'workspace': G.carve_arena((WS_BYTES,), torch.uint8, 'cpu', sentinel)}
        for name, want in expected.items():
            t[name] = _carve_np(want, sentinel, False)
            t[name].payload.numpy()[masks[name]] = want[masks[name]]
        if mutate is not None:
            mutate(t, sentinel, expected)
        return t

    return run, {'highres': x}, list(expected), expected, masks


def decode_launch(ndim, span, mutate=None):
    _, lo, maps, _, back = _reference(ndim)
    inputs = {'lowres': lo, **{f'map{k}': m for k, m in enumerate(maps)}}
    expected = {'highres': back}
    masks = G.decode_masks(back.shape, lo.shape, _region(ndim, span), ndim)

    def run(sentinel):
        t = {name: _carve_np(a, sentinel, True) for name, a in inputs.items()}
        t['workspace'] = G.carve_arena((WS_BYTES,), torch.uint8, 'cpu', sentinel)
        t['highres'] = _carve_np(back, sentinel, False)
        t['highres'].payload.numpy()[masks['highres']] = back[masks['highres']]
        if mutate is not None:
            mutate(t, sentinel, expected)
        return t

    return run, inputs, ['highres'], expected, masks


# ---------------------------------------------------------------------------------------------
# carve
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype,shift', [(torch.uint8, 0), (torch.uint8, 1), (torch.uint16, 0), (torch.uint16, 2),
                                         (torch.uint16, 8), (torch.int32, 8)])
def test_carve_layout(dtype, shift):
    arena, payload = G.carve((3, 5, 7), dtype, 'cpu', 0xA5, shift)
    item = payload.element_size()
    assert arena.dtype == torch.uint8 and arena.numel() == 2 * G.GUARD + shift + 105 * item
    assert bool((arena == 0xA5).all())
    assert payload.is_contiguous() and tuple(payload.shape) == (3, 5, 7) and payload.dtype == dtype
    assert payload.data_ptr() == arena.data_ptr() + G.GUARD + shift
    assert (payload.data_ptr() - shift) % G.ALIGN == 0
    payload.view(torch.uint8).fill_(1)
    a = arena.numpy()
    assert (a[:G.GUARD + shift] == 0xA5).all() and (a[G.GUARD + shift + 105 * item:] == 0xA5).all()
    assert (a[G.GUARD + shift:G.GUARD + shift + 105 * item] == 1).all()


def test_carve_rejects_a_shift_off_the_item_size():
    with pytest.raises(ValueError):
        G.carve((4,), torch.uint16, 'cpu', 0xA5, shift=1)


def test_carve_empty_payload():
    arena, payload = G.carve((0,), torch.uint8, 'cpu', 0x5A)
    assert payload.numel() == 0 and arena.numel() == 2 * G.GUARD


# ---------------------------------------------------------------------------------------------
# the honest writer passes
# ---------------------------------------------------------------------------------------------

SPANS = {3: [None, (1, 3), (0, 2), (3, 5), (-4, 99), (3, 3)], 2: [None, (5, 11), (0, 7), (9, 16), (-1, 40), (8, 2)]}


@pytest.mark.parametrize('ndim', [3, 2])
@pytest.mark.parametrize('which', range(6))
def test_oracle_writer_passes(ndim, which):
    span = SPANS[ndim][which]
    G.check_launch_pair(*encode_launch(ndim, span))
    G.check_launch_pair(*decode_launch(ndim, span))


def test_region_masks_match_the_slab_planes():
    """The decode mask of a z region is highres planes [2 r0, min(2 r1, D)), what slabs.py returns."""
    _, lo, _, _, back = _reference(3)
    D = back.shape[1]
    for r0, r1 in [(0, 2), (1, 3), (3, 5), (0, 5)]:
        m = G.decode_masks(back.shape, lo.shape, _region(3, (r0, r1)), 3)['highres']
        want = np.zeros(back.shape, bool)
        want[:, 2 * r0:min(2 * r1, D)] = True
        assert np.array_equal(m, want)


# ---------------------------------------------------------------------------------------------
# every wrong writer is flagged, with the tensor named
# ---------------------------------------------------------------------------------------------

def _past_end_of_map(t, s, exp):
    c = t['map6']
    c.arena.numpy()[G.GUARD + c.nbytes:G.GUARD + c.nbytes + 2] = 0x11


def _before_lowres(t, s, exp):
    t['lowres'].arena.numpy()[G.GUARD - 2:G.GUARD] = 0x11


def _plane_outside_right(t, s, exp):
    t['map3'].payload.numpy()[:, 3] = exp['map3'][:, 3]


def _plane_outside_wrong(t, s, exp):
    t['map0'].payload.numpy()[:, 0] = exp['map0'][:, 0] + 1


def _owned_copies_guard(t, s, exp):
    t['lowres'].payload.numpy()[0, 1, 0, 0, 0] = s * 257


def _owned_differs(t, s, exp):
    t['map2'].payload.numpy()[0, 1, 2, 3, 0] = exp['map2'][0, 1, 2, 3, 0] + (1 if s == G.SENTINELS[1] else 0)


def _input_modified(t, s, exp):
    t['highres'].payload.view(torch.uint8).view(-1).numpy()[12345] ^= 1


def _workspace_overrun(t, s, exp):
    t['workspace'].arena.numpy()[G.GUARD + WS_BYTES] = 0


ENCODE_MUTANTS = [
    ('past-end-of-map', _past_end_of_map, {('guard', 'map6')}),
    ('before-lowres', _before_lowres, {('guard', 'lowres')}),
    ('plane-outside-box-right-values', _plane_outside_right, {('unowned', 'map3')}),
    ('plane-outside-box-wrong-values', _plane_outside_wrong, {('unowned', 'map0')}),
    ('owned-copies-guard-byte', _owned_copies_guard, {('value', 'lowres'), ('nondeterministic', 'lowres')}),
    ('owned-differs-between-runs', _owned_differs, {('value', 'map2'), ('nondeterministic', 'map2')}),
    ('input-modified', _input_modified, {('input', 'highres')}),
    ('workspace-overrun', _workspace_overrun, {('guard', 'workspace')}),
]


@pytest.mark.parametrize('name,mutate,want', ENCODE_MUTANTS, ids=[m[0] for m in ENCODE_MUTANTS])
def test_wrong_encode_writer_is_flagged(name, mutate, want):
    with pytest.raises(G.GuardError) as e:
        G.check_launch_pair(*encode_launch(3, (1, 3), mutate))
    got = {(check, tensor) for check, tensor, _ in e.value.failures}
    assert got == want, str(e.value)
    for _, tensor in want:
        assert tensor in str(e.value)


def _dec_plane_outside_right(t, s, exp):
    t['highres'].payload.numpy()[:, 6] = exp['highres'][:, 6]  # region (1, 3) owns planes 2..5


def _dec_plane_outside_wrong(t, s, exp):
    t['highres'].payload.numpy()[:, 1] = exp['highres'][:, 1] ^ 0x55


def _dec_past_end(t, s, exp):
    c = t['highres']
    c.arena.numpy()[G.GUARD + c.nbytes] = 0


def _dec_owned_differs(t, s, exp):
    t['highres'].payload.numpy()[1, 2, 3, 4, 0] = exp['highres'][1, 2, 3, 4, 0] ^ (s & 1)


def _dec_input_map_modified(t, s, exp):
    t['map4'].payload.view(torch.uint8).view(-1).numpy()[7] ^= 0x80


DECODE_MUTANTS = [
    ('plane-outside-box-right-values', _dec_plane_outside_right, {('unowned', 'highres')}),
    ('plane-outside-box-wrong-values', _dec_plane_outside_wrong, {('unowned', 'highres')}),
    ('past-end-of-highres', _dec_past_end, {('guard', 'highres')}),
    ('owned-differs-between-runs', _dec_owned_differs, {('value', 'highres'), ('nondeterministic', 'highres')}),
    ('input-map-modified', _dec_input_map_modified, {('input', 'map4')}),
]


@pytest.mark.parametrize('name,mutate,want', DECODE_MUTANTS, ids=[m[0] for m in DECODE_MUTANTS])
def test_wrong_decode_writer_is_flagged(name, mutate, want):
    with pytest.raises(G.GuardError) as e:
        G.check_launch_pair(*decode_launch(3, (1, 3), mutate))
    assert {(check, tensor) for check, tensor, _ in e.value.failures} == want, str(e.value)


def test_wrong_image_writer_is_flagged():
    """Rows (5, 11) of the image: a row outside the box in the last map, right values."""
    def mutate(t, s, exp):
        t['map2'].payload.numpy()[:, 11] = exp['map2'][:, 11]
    with pytest.raises(G.GuardError) as e:
        G.check_launch_pair(*encode_launch(2, (5, 11), mutate))
    assert {(c, n) for c, n, _ in e.value.failures} == {('unowned', 'map2')}


def test_empty_region_flags_any_write():
    def mutate(t, s, exp):
        t['map5'].payload.numpy()[0, 0, 0, 0, 0] = exp['map5'][0, 0, 0, 0, 0]
    with pytest.raises(G.GuardError) as e:
        G.check_launch_pair(*encode_launch(3, (3, 3), mutate))
    assert {(c, n) for c, n, _ in e.value.failures} == {('unowned', 'map5')}


def test_empty_region_flags_a_workspace_write():
    def mutate(t, s, exp):
        t['workspace'].payload[5] = 0
    run, inputs, outputs, expected, masks = encode_launch(3, (3, 3), mutate)
    G.check_launch_pair(run, inputs, outputs, expected, masks)  # scratch unless the launch owns nothing
    with pytest.raises(G.GuardError) as e:
        G.check_launch_pair(run, inputs, outputs, expected, masks, untouched=('workspace',))
    assert {(c, n) for c, n, _ in e.value.failures} == {('unowned', 'workspace')}


def test_failure_report_names_index_and_offset():
    with pytest.raises(G.GuardError) as e:
        G.check_launch_pair(*encode_launch(3, (1, 3), _before_lowres))
    assert 'lowres: 2 guard bytes changed' in str(e.value) and '-2, -1' in str(e.value)
    with pytest.raises(G.GuardError) as e:
        G.check_launch_pair(*encode_launch(3, (1, 3), _plane_outside_right))
    assert '(0, 3, 0, 0, 0) at byte +' in str(e.value)


# ---------------------------------------------------------------------------------------------
# the masks on their own, against the oracle's shapes
# ---------------------------------------------------------------------------------------------

MASK_SHAPES = [(1, 6, 8, 10, 1), (1, 7, 9, 11, 1), (2, 6, 9, 8, 1), (1, 7, 8, 9, 2), (1, 5, 6, 7, 1),
               (1, 8, 10, 1), (1, 9, 11, 1), (2, 8, 11, 1), (1, 9, 10, 3)]


@pytest.mark.parametrize('shape', MASK_SHAPES, ids=['x'.join(map(str, s)) for s in MASK_SHAPES])
def test_slab_masks_partition_every_tensor(shape):
    ndim = len(shape) - 2
    ns = oracle.volume if ndim == 3 else oracle.image
    x = np.zeros(shape, np.uint8)
    lo, (maps, dims) = ns.encode(OP.mean_predictions_fn(0, ndim), ns.encode_values_uint8, x, padding=0)
    E = lo.shape[1:1 + ndim]
    assert tuple(dims) == tuple((s + 1) % 2 for s in shape[1:1 + ndim])
    whole = G.encode_masks(lo.shape, [m.shape for m in maps], None, ndim)
    assert all(m.all() for m in whole.values()) and len(whole) == 1 + len(maps)
    assert G.decode_masks(shape, lo.shape, None, ndim)['highres'].all()
    cuts = sorted({0, 1, E[0] // 2, E[0] - 1, E[0]})
    slabs = [[(a, b)] + [(0, e) for e in E[1:]] for a, b in zip(cuts[:-1], cuts[1:])]
    slabs[0][0] = (-3, slabs[0][0][1])       # overshoot clamps
    slabs[-1][0] = (slabs[-1][0][0], E[0] + 7)
    enc = [G.encode_masks(lo.shape, [m.shape for m in maps], r, ndim) for r in slabs]
    for name in whole:
        count = sum(m[name].astype(np.int32) for m in enc)
        assert (count == 1).all(), name
    count = sum(G.decode_masks(shape, lo.shape, r, ndim)['highres'].astype(np.int32) for r in slabs)
    assert (count == 1).all()


def test_masks_restrict_every_axis():
    lo_shape, hi_shape = (1, 4, 5, 6, 1), (1, 7, 10, 11, 1)
    m = G.decode_masks(hi_shape, lo_shape, [(1, 3), (2, 4), (0, 2)], 3)['highres']
    want = np.zeros(hi_shape, bool)
    want[:, 2:6, 4:8, 0:4] = True
    assert np.array_equal(m, want)
    e = G.encode_masks(lo_shape, [(1, 3, 4, 6, 1)], [(1, 4), (2, 5), (0, 2)], 3)
    want = np.zeros((1, 3, 4, 6, 1), bool)
    want[:, 1:3, 2:4, 0:2] = True
    assert np.array_equal(e['map0'], want) and e['lowres'].sum() == 3 * 3 * 2
    assert not G.encode_masks(lo_shape, [], [(2, 2), (0, 5), (0, 6)], 3)['lowres'].any()


# ---------------------------------------------------------------------------------------------
# box copies and outputs judged by a predicate (the helpers of the C-ABI guard modules)
# ---------------------------------------------------------------------------------------------

def test_copy_box_mask_is_the_box():
    m = G.copy_box_mask((2, 5, 6, 7, 3), (1, 0, 4), (3, 2, 3), 3)
    want = np.zeros((2, 5, 6, 7, 3), bool)
    want[:, 1:4, 0:2, 4:7, :] = True
    assert np.array_equal(m, want)
    m2 = G.copy_box_mask((3, 4, 9, 1), (2, 1), (2, 0), 2)
    assert m2.shape == (3, 4, 9, 1) and not m2.any()  # an empty extent owns nothing


def _box_launch(extra=None):
    """A 'box copy' of a float32 source into dst[:, 1:3, 2:5], written by numpy into CPU arenas."""
    src = np.arange(2 * 2 * 3, dtype=np.float32).reshape(2, 2, 3, 1) + 0.5
    shape = (2, 4, 6, 1)
    mask = G.copy_box_mask(shape, (1, 2), (2, 3), 2)
    want = np.zeros(shape, np.float32)
    want[:, 1:3, 2:5] = src

    def run(sentinel):
        t = {'src': G.fill(G.carve_arena(src.shape, torch.float32, 'cpu', sentinel), src),
             'dst': G.carve_arena(shape, torch.float32, 'cpu', sentinel)}
        t['dst'].payload.numpy()[:, 1:3, 2:5] = src
        if extra is not None:
            extra(t, sentinel)
        return t

    return run, {'src': src}, ['dst'], {'dst': want}, {'dst': mask}, want


def test_box_copy_passes_and_a_store_past_the_box_is_unowned():
    run, inputs, outputs, expected, masks, _ = _box_launch()
    G.check_launch_pair(run, inputs, outputs, expected, masks)

    def spill(t, sentinel):  # one element past the box's x end, inside dst
        t['dst'].payload.numpy()[1, 2, 5, 0] = 7.0

    run, inputs, outputs, expected, masks, _ = _box_launch(spill)
    with pytest.raises(G.GuardError) as e:
        G.check_launch_pair(run, inputs, outputs, expected, masks)
    assert [(c, n) for c, n, _ in e.value.failures] == [('unowned', 'dst')] * 2


def test_predicate_replaces_only_the_value_comparison():
    run, inputs, outputs, _, masks, want = _box_launch()
    near = lambda v: np.abs(v.astype(np.float64) - want) > 0.25  # noqa: E731
    seen = []

    def judge(v):
        seen.append((v.dtype, v.shape))
        return near(v)

    G.check_launch_pair(run, inputs, outputs, {}, masks, predicates={'dst': (np.float32, judge)})
    assert seen == [(np.dtype(np.float32), (2, 4, 6, 1))] * 2

    def off_by_a_little(t, sentinel):  # within the bound: passes; bytewise it would not
        t['dst'].payload.numpy()[0, 1, 2, 0] += 0.125

    run, inputs, outputs, expected, masks, _ = _box_launch(off_by_a_little)
    G.check_launch_pair(run, inputs, outputs, {}, masks, predicates={'dst': (np.float32, near)})
    with pytest.raises(G.GuardError) as e:
        G.check_launch_pair(run, inputs, outputs, expected, masks)
    assert {(c, n) for c, n, _ in e.value.failures} == {('value', 'dst')}

    def off_by_a_lot(t, sentinel):
        t['dst'].payload.numpy()[0, 1, 2, 0] += 1.0

    run, inputs, outputs, _, masks, _ = _box_launch(off_by_a_lot)
    with pytest.raises(G.GuardError) as e:
        G.check_launch_pair(run, inputs, outputs, {}, masks, predicates={'dst': (np.float32, near)})
    assert [(c, n, k) for c, n, k in e.value.failures] == [('value', 'dst', 1)] * 2

    def spill_and_depend(t, sentinel):  # the other checks still apply to a predicate output
        t['dst'].payload.numpy()[1, 0, 0, 0] = 3.0
        t['dst'].payload.numpy()[0, 1, 2, 0] += 0.001 * sentinel

    run, inputs, outputs, _, masks, _ = _box_launch(spill_and_depend)
    with pytest.raises(G.GuardError) as e:
        G.check_launch_pair(run, inputs, outputs, {}, masks, predicates={'dst': (np.float32, near)})
    assert {(c, n) for c, n, _ in e.value.failures} == {('unowned', 'dst'), ('nondeterministic', 'dst')}
