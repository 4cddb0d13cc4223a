"""Guard bands, region exactness and run-to-run determinism for every fused codec family.

Each case is one encode and one decode through ``_nd.fused_plan`` + ``_nd.fused_encode_into`` /
``_nd.fused_decode_into`` (the product's two entry points) with EVERY tensor the kernels touch --
highres, lowres, each map, the workspace at exactly ``workspace_bytes()`` -- carved from arenas the
test owns (guard_spec.py), run twice on two sentinel fills.  Checked per launch: (a) guards, pointer
shifts and inputs untouched, (b) nothing outside the region's box written, (c) the box bit-equal
to the reference in both runs, (d) the two runs identical; and the launch's name, so no case passes
by silently running another kernel.

The matrix is ROWS of test_gpu_routing.py (imported, not copied) plus, per family, a sibling whose
restricted axis is odd (``dims`` = 0: the parity maps are one entry shorter), the image
LinearPredictor rows of the generic row kernel (``fuse_lin2d``), and a volume region that also
restricts y and x.  Reference: the oracle (mean / f32 rows); for bf16x2 rows, which the oracle does
not equal bit for bit by design, the same request through the two-pass path
(KMP_DISABLE_LINEAR_FUSED=1) in plain tensors, whose out-of-range cells test_gpu_linear_casts.py pins
to the specification.  A reference is computed once per (row, pattern) at
the largest batch the row runs; smaller batches are its leading items (every step of the codec is
per batch item)."""

import numpy as np
import pytest
import torch

import oracle
from oracle import predictors as OP
import guard_spec as G
from test_gpu_routing import ROWS, _family, _predictor

pytestmark = pytest.mark.gpu

U8, U16, I32 = np.uint8, np.uint16, np.int32
NP2T = {U8: torch.uint8, U16: torch.uint16, I32: torch.int32}
CODER = {U8: 'uint8', U16: 'uint16', I32: 'raw'}

# Siblings of the routing rows whose restricted axis (z of a volume, the rows of an image) is odd, so
# ``dims`` is 0 there and the parity maps end one entry before E; one per family, each still taken
# by that family (W stays even and a multiple of 16 bytes; the *_geometry rules on H and D hold).
# fast3d, linear3d and linear3dp need none: their routing rows already have an odd depth.
SIBLINGS = [
    ('odd-vol-u16-p0', (2, 11, 16, 64, 1), U16, 'mean', 0, {}, None, 'wave3d_encode', 'wave3d_decode'),
    ('odd-vol-u8-p0', (2, 11, 16, 64, 1), U8, 'mean', 0, {}, None, 'wave3d_encode', 'wave3d_decode'),
    ('odd-vol-u16-p1', (2, 11, 16, 64, 1), U16, 'mean', 1, {}, None, 'wave3dp_encode', 'wave3dp_decode'),
    ('odd-vol-u8-p2', (2, 11, 16, 64, 1), U8, 'mean', 2, {}, None, 'wave3dp_encode', 'wave3dp_decode'),
    ('odd-vol-u16-p2', (2, 11, 16, 64, 1), U16, 'mean', 2, {}, None, 'wave3dr_encode', 'wave3dr_decode'),
    ('odd-vol-i32-p0', (2, 7, 10, 32, 1), I32, 'mean', 0, {}, None, 'wave3d32_encode', 'wave3d32_decode'),
    ('odd-vol-u8-c3', (1, 7, 16, 32, 3), U8, 'mean', 0, {}, None, 'encode_generic', 'decode_generic'),
    ('odd-vol-lin-f32-p0', (1, 7, 32, 32, 1), U16, 'f32', 0, {}, None, 'linear3y_encode', 'linear3y_decode'),
    ('odd-vol-lin-mfma-p0', (2, 15, 32, 32, 1), U16, 'bf16x2', 0, {}, None, 'linear3m_encode', 'linear3m_decode'),
    ('odd-vol-lin-mfma-p1', (1, 7, 32, 64, 1), U16, 'bf16x2', 1, {}, None, 'linear3pm_encode', 'linear3pm_decode'),
    ('odd-img-u8-p0', (2, 31, 64, 1), U8, 'mean', 0, {}, None, 'wave2d_encode', 'wave2d_decode'),
    ('odd-img-u16-p1', (2, 31, 64, 1), U16, 'mean', 1, {}, None, 'wave2dr_encode', 'wave2dr_decode'),
    ('odd-img-u8-p2', (2, 31, 64, 1), U8, 'mean', 2, {}, None, 'wave2dr_encode', 'wave2dr_decode'),
    ('odd-img-lin-f32-p0', (3, 63, 64, 1), U16, 'f32', 0, {}, None, 'wave2d_encode', 'wave2d_decode'),
    ('odd-img-u8-c3', (2, 15, 32, 3), U8, 'mean', 0, {}, None, 'encode_generic', 'decode_generic'),
    # 8-bit samples on the f32 / matrix-core p = 1 kernels: their highres segments are 8 bytes
    ('vol-lin-f32-p1-u8', (2, 9, 14, 32, 1), U8, 'f32', 1, {}, None, 'linear3dp_encode', 'linear3dp_decode'),
    ('vol-lin-mfma-p1-u8', (1, 7, 32, 64, 1), U8, 'bf16x2', 1, {}, None, 'linear3pm_encode', 'linear3pm_decode'),
]

# Images, one channel, f32 LinearPredictor, p <= 1, odd width (no wave kernel): the generic row kernel
# computes the cells itself (fuse_lin2d, kmp_codec_generic.hip)
LIN2D = [
    (f'lin2d-{np.dtype(dt).name}-p{p}-{"x".join(map(str, shape[1:3]))}', shape, dt, 'f32', p, {}, None,
     'encode_generic', 'decode_generic')
    for dt in (U8, U16) for p in (0, 1) for shape in ((2, 31, 45, 1), (1, 7, 9, 1))
]

MATRIX = list(ROWS) + SIBLINGS + LIN2D
ROW_BY_ID = {r[0]: r for r in MATRIX}
assert len(ROW_BY_ID) == len(MATRIX)

# Highres alignment each family asks of ptrs_aligned (bytes; 'seg' = 8 * sizeof(T), the 8-sample row
# segment of linear3dp / linear3pm); lowres and the maps: 8 bytes at most everywhere (4 * sizeof(T)
# for the two 'seg' families)
HI_ALIGN = {'wave3d': 16, 'wave3d32': 16, 'wave3dp': 16, 'wave3dr': 16, 'fast3d': 16, 'linear3d': 16,
            'linear3y': 16, 'linear3m': 16, 'linear3dp': 'seg', 'linear3pm': 'seg', 'wave2d': 16,
            'wave2dr': 16, 'fast2d': 16, 'generic': 1}
# families whose B = 16 + region case the matrix adds (the block remap meets the region offset)
B16_FAMILIES = ('wave3d', 'wave3dp', 'wave3dr', 'wave3d32', 'linear3y', 'linear3d', 'linear3dp', 'linear3m',
                'linear3pm')
REQUIRED = ('wave3d', 'wave3dp', 'wave3dr', 'wave3d32', 'fast3d', 'linear3y', 'linear3d', 'linear3dp', 'linear3m',
            'linear3pm', 'wave2d', 'wave2dr', 'fast2d', 'generic')

# (family, direction, a non-empty proper region?, B % 8 == 0) of every launch this module made
SEEN = set()

_REF = {}
_PRED = {}


def _name(family, direction):
    return f'{direction}_generic' if family == 'generic' else f'{family}_{direction}'


def _ns(kom, ndim):
    return (kom.volume, oracle.volume) if ndim == 3 else (kom.image, oracle.image)


def _bmax(row):
    return 16 if len(row[1]) == 5 and _family(row[7]) in B16_FAMILIES else 8


def _pattern(shape, dtype, pattern):
    info = np.iinfo(dtype)
    if pattern in ('random', 'clamp'):  # full range, as routing uses
        return np.random.default_rng(40).integers(info.min, info.max + 1, size=shape, dtype=np.int64).astype(dtype)
    if pattern == 'max':
        return np.full(shape, info.max, dtype)
    assert pattern == 'checker'  # 0 / max by coordinate parity: the largest residuals, the coder's wrap
    nsp = len(shape) - 2
    par = sum(np.arange(shape[1 + a]).reshape([-1 if ax == 1 + a else 1 for ax in range(len(shape))])
              for a in range(nsp)) % 2
    return np.broadcast_to(par * info.max, shape).astype(dtype)


def _clamp_weights(p, ndim, dtype):
    """Weights near the mean with biases spread evenly over [-1.2 max, 1.2 max]: of the K predictions
    some fall below 0, some above max, some cross an edge of the range."""
    n, k = (2 * p + 2) ** ndim, 19 if ndim == 3 else 5
    rng = np.random.default_rng(43)
    w = ((1.0 / n) * (1.0 + 0.3 * rng.standard_normal((n, k)))).astype(np.float32)
    b = (rng.permutation(np.linspace(-1.2, 1.2, k)) * np.iinfo(dtype).max).astype(np.float32)
    return w, b


def _assert_both_clamps(ons, x, w, b, p, dtype, split):
    """From the float64 value alone (of the bf16x2 split weights for ``split``), with the 1e-5 margin
    that bounds either arithmetic's distance from it: some predictions lie at or below -1, some at or
    above max + 1, some inside the range, whichever arithmetic evaluates them."""
    lowres = ons.pad_neighborhood(ons.lowres_from_highres(ons.pad_highres(x)[0]), p)
    feats = ons.features_from_lowres(lowres, p)
    v = OP.linear_bf16x2_split(feats, w, b) if split else OP.linear_predictions(feats, w, b, dtype)[0]
    nd = feats.ndim - 2
    scale = np.tensordot(np.moveaxis(np.abs(feats.astype(np.float64)), nd, -1), np.abs(w.astype(np.float64)),
                         axes=([-1], [0]))
    m = 1e-5 * (np.moveaxis(scale, -1, nd) + np.abs(b.astype(np.float64)).reshape(-1, 1))
    top = np.iinfo(dtype).max
    assert (v <= -1.0 - m).any() and (v >= top + 1.0 + m).any() and ((v > m) & (v < top - m)).any()


def _predictor_for(kom, row, pattern):
    _, shape, dtype, kind, p, *_ = row
    ndim = len(shape) - 2
    key = (kind, p, ndim, np.dtype(dtype).name, pattern == 'clamp')
    if key not in _PRED:
        if pattern == 'clamp':
            assert kind in ('f32', 'bf16x2')
            _PRED[key] = kom.LinearPredictor(*_clamp_weights(p, ndim, dtype), p, ndim, arith=kind)
        else:
            _PRED[key] = _predictor(kom, kind, p, ndim, dtype)
    return _PRED[key]


def _reference(kom, kmp_opt, row, pattern):
    """{'x', 'lowres', 'maps', 'dims', 'back'} at the row's largest batch, computed once."""
    rid, shape, dtype, kind, p, *_ = row
    key = (rid, pattern)
    if key in _REF:
        return _REF[key]
    ndim = len(shape) - 2
    ns, ons = _ns(kom, ndim)
    x = _pattern((_bmax(row),) + tuple(shape[1:]), dtype, pattern)
    pred = _predictor_for(kom, row, pattern)
    if kind in ('f32', 'bf16x2') and pattern == 'clamp':
        _assert_both_clamps(ons, x[:shape[0]], pred.weights.numpy(), pred.bias.numpy(), p, dtype, kind == 'bf16x2')
    if kind == 'bf16x2':  # the two-pass path on the same arithmetic, in plain tensors
        kmp_opt('KMP_DISABLE_LINEAR_FUSED', 1)
        last = lambda: kom._lib.lib.kmp_last_launch().decode()  # noqa: E731
        lo, (maps, dims) = ns.encode(pred, getattr(ns, 'encode_values_' + CODER[dtype]), x, padding=p)
        assert last() == 'encode_generic'
        back = ns.decode(pred, getattr(ns, 'decode_values_' + CODER[dtype]), lo, (maps, dims), padding=p)
        assert last() == 'decode_generic'
        kmp_opt('KMP_DISABLE_LINEAR_FUSED', None)
    else:
        if kind == 'mean':
            fn = OP.mean_predictions_fn(p, ndim)
        else:
            w, b = pred.weights.numpy(), pred.bias.numpy()
            fn = OP.linear_predictions_fn(p, w, b, ndim)
            if pattern == 'clamp':  # from the oracle's predictions alone: both clamps occur
                lowres = ons.pad_neighborhood(ons.lowres_from_highres(ons.pad_highres(x[:shape[0]])[0]), p)
                v = OP.linear_fma_chain(ons.features_from_lowres(lowres, p), w, b)
                top = np.iinfo(dtype).max
                assert (v <= -1.0).any() and (v >= top + 1.0).any() and ((v > 0) & (v < top)).any()
        lo, (maps, dims) = ons.encode(fn, getattr(ons, 'encode_values_' + CODER[dtype]), x, padding=p)
        back = ons.decode(fn, getattr(ons, 'decode_values_' + CODER[dtype]), lo, (maps, dims), padding=p)
    assert np.array_equal(back, x), 'the reference itself is not lossless'
    _REF[key] = {'x': x, 'lowres': np.ascontiguousarray(lo), 'maps': [np.ascontiguousarray(m) for m in maps],
                 'dims': tuple(int(d) for d in dims), 'back': np.ascontiguousarray(back)}
    return _REF[key]


def _spans(E0):
    """Spans of the restricted axis: strictly inside with an odd begin, touching the start, touching
    the end, over both ends (behaves as clamped: the whole axis), empty."""
    return {'inside': (1, E0 - 1), 'start': (0, max(1, E0 // 2)), 'end': (E0 // 2, E0),
            'over': (-2, E0 + 3), 'empty': (E0 - 1, 1)}


def _expected_family(row, direction, region, E, shift):
    """The family the dispatch table gives this variant of ``row`` (each rule is the line of the
    family's try_* / *_geometry it restates)."""
    fam = _family(row[7 if direction == 'encode' else 8])
    dtype = row[2]
    if region is not None:
        if any(b > 0 or e < ext for (b, e), ext in zip(region[1:], E[1:])) and len(E) == 3:
            return 'generic'  # region_span: a one-pass volume family takes z slabs only
        if len(E) == 2 and (region[1][0] > 0 or region[1][1] < E[1]):
            return 'generic'  # ... an image family row ranges only
        if fam == 'fast2d':
            return 'generic'  # f2::geometry refuses every region (kmp_codec_fast2d.hip)
    if shift is not None:
        which, nbytes = shift
        if which == 'highres':
            align = HI_ALIGN[fam]
            align = 8 * np.dtype(dtype).itemsize if align == 'seg' else align
            if nbytes % align:
                return 'generic'
    return fam


class Case:
    def __init__(self, B, span=None, pattern='random', shift=None, region=None, claim=None):
        self.B, self.span, self.pattern, self.shift, self.region = B, span, pattern, shift, region
        self.claim = claim  # the box the masks are built from, when the test lies about it on purpose

    def __repr__(self):
        return f'B={self.B} span={self.span} region={self.region} pattern={self.pattern} shift={self.shift}'


def run_case(kom, kmp_opt, row, case):
    """One encode and one decode of ``row`` under check_launch_pair; returns the launch names."""
    from kompressor_amd import _nd, _lib
    rid, shape, dtype, _, p, options, _, _, _ = row
    for name, value in options.items():
        kmp_opt(name, value)
    ndim = len(shape) - 2
    ns, _ = _ns(kom, ndim)
    ref = _reference(kom, kmp_opt, row, case.pattern)
    B = case.B
    x, lo, back, dims = ref['x'][:B], ref['lowres'][:B], ref['back'][:B], ref['dims']
    maps = [m[:B] for m in ref['maps']]
    E = lo.shape[1:1 + ndim]
    region = case.region
    if region is None and case.span is not None:
        region = [_spans(E[0])[case.span]] + [(0, int(e)) for e in E[1:]]
    claim = region if case.claim is None else case.claim
    box = G.clamp_box(region, E)
    empty = any(e <= b for b, e in box)
    proper = region is not None and not empty and box != [(0, int(e)) for e in E]
    pred = _predictor_for(kom, row, case.pattern)
    td = NP2T[dtype]
    sh = {'highres': 0, 'lowres': 0, f'map{len(maps) - 1}': 0}
    if case.shift is not None:
        sh[case.shift[0] if case.shift[0] != 'lastmap' else f'map{len(maps) - 1}'] = case.shift[1]
    last = lambda: kom._lib.lib.kmp_last_launch().decode()  # noqa: E731
    names = {}

    def carve(arr, name, s, filled):
        c = G.carve_arena(arr.shape, NP2T[arr.dtype.type], 'cuda', s, sh.get(name, 0))
        return G.fill(c, arr) if filled else c

    def note(direction):  # after each launch: the family the table promises served it
        names[direction] = last()
        SEEN.add((_family(names[direction]), direction, proper, B % 8 == 0))
        want = _name(_expected_family(row, direction, region, E, case.shift), direction)
        assert names[direction] == want, f'{rid} {case}: launched {names[direction]}, expected {want}'

    # ---- encode ----
    plan = _nd.fused_plan(pred, getattr(ns, 'encode_values_' + CODER[dtype]), p, td, ndim, _lib.ENCODE)
    assert plan is not None
    outs = {'lowres': lo, **{f'map{k}': m for k, m in enumerate(maps)}}

    def run_encode(s):
        t = {'highres': carve(x, 'highres', s, True)}
        t.update({name: carve(a, name, s, False) for name, a in outs.items()})
        need = _nd.workspace_bytes(t['highres'].payload, pred, ndim)
        t['workspace'] = G.carve_arena((need,), torch.uint8, 'cuda', s)
        got = _nd.fused_encode_into(t['highres'].payload, plan[0], plan[1], t['lowres'].payload,
                                    [t[f'map{k}'].payload for k in range(len(maps))], ndim, region=region,
                                    workspace=t['workspace'].payload)
        assert tuple(got) == dims
        if not empty:  # (an empty box returns before any launch: there is no name to read)
            note('encode')
        return t

    G.check_launch_pair(run_encode, {'highres': x}, list(outs), outs,
                        G.encode_masks(lo.shape, [m.shape for m in maps], claim, ndim),
                        untouched=('workspace',) if empty else ())

    # ---- decode (inputs: the reference's encode) ----
    plan = _nd.fused_plan(pred, getattr(ns, 'decode_values_' + CODER[dtype]), p, td, ndim, _lib.DECODE)
    assert plan is not None

    def run_decode(s):
        t = {name: carve(a, name, s, True) for name, a in outs.items()}
        t['highres'] = carve(back, 'highres', s, False)
        need = _nd.workspace_bytes(t['highres'].payload, pred, ndim)
        t['workspace'] = G.carve_arena((need,), torch.uint8, 'cuda', s)
        _nd.fused_decode_into(t['lowres'].payload, [t[f'map{k}'].payload for k in range(len(maps))], dims, plan[0],
                              plan[1], t['highres'].payload, ndim, region=region, workspace=t['workspace'].payload)
        if not empty:
            note('decode')
        return t

    G.check_launch_pair(run_decode, outs, ['highres'], {'highres': back},
                        G.decode_masks(back.shape, lo.shape, claim, ndim),
                        untouched=('workspace',) if empty else ())

    return names


def _own(row):
    return row[1][0]


IDS = [r[0] for r in MATRIX]


@pytest.mark.parametrize('rid', IDS)
def test_guard_regions(kom, kmp_opt, rid):
    """The row's own batch: whole frame and every kind of region."""
    row = ROW_BY_ID[rid]
    for span in (None, 'inside', 'start', 'end', 'over', 'empty'):
        run_case(kom, kmp_opt, row, Case(_own(row), span))


@pytest.mark.parametrize('rid', IDS)
def test_guard_batches(kom, kmp_opt, rid):
    """B = 8 takes the XCD-contiguous block order; the volume wave and linear families also run
    B = 16 with a region (the block remap and the region offset in one launch)."""
    row = ROW_BY_ID[rid]
    run_case(kom, kmp_opt, row, Case(8, None))
    run_case(kom, kmp_opt, row, Case(8, 'inside'))
    if _bmax(row) == 16:
        run_case(kom, kmp_opt, row, Case(16, 'end'))
        run_case(kom, kmp_opt, row, Case(16, 'inside'))


@pytest.mark.parametrize('rid', IDS)
def test_guard_patterns(kom, kmp_opt, rid):
    """All-max, the 0 / max checkerboard and (LinearPredictor rows, either arithmetic) predictions
    that leave [0, max]."""
    row = ROW_BY_ID[rid]
    for pattern in ('max', 'checker') + (('clamp',) if row[3] in ('f32', 'bf16x2') else ()):
        run_case(kom, kmp_opt, row, Case(_own(row), None, pattern))
        run_case(kom, kmp_opt, row, Case(_own(row), 'end', pattern))


@pytest.mark.parametrize('rid', IDS)
def test_guard_pointer_shifts(kom, kmp_opt, rid):
    """Pointers off their natural alignment: 8 bytes on lowres or the last map keep the family; 8 bytes
    on highres leave only the 8-bit linear3dp / linear3pm kernels eligible; one element on highres
    leaves none.  The bits stay the same."""
    row = ROW_BY_ID[rid]
    item = np.dtype(row[2]).itemsize
    for shift in (('lowres', 8), ('lastmap', 8), ('highres', 8), ('highres', item)):
        run_case(kom, kmp_opt, row, Case(_own(row), None, shift=shift))


YX_REGIONS = [
    ('vol-u16-p1', [(1, 5), (2, 7), (3, 29)]),
    ('vol-u16-p1', [(0, 6), (0, 8), (5, 40)]),
    ('vol-u16-p1', [(0, 6), (3, 8), (0, 32)]),
    ('vol-lin-f32-p1', [(1, 4), (1, 6), (0, 9)]),
    ('vol-lin-mfma-p0', [(3, 8), (5, 16), (7, 15)]),
    ('img-u8-p2', [(3, 12), (5, 31)]),
    ('lin2d-uint16-p1-31x45', [(5, 16), (1, 22)]),
]


@pytest.mark.parametrize('rid,region', YX_REGIONS, ids=[f'{r}-{i}' for i, (r, _) in enumerate(YX_REGIONS)])
def test_guard_region_on_every_axis(kom, kmp_opt, rid, region):
    """A box that restricts y / x too: no one-pass family takes it (region_span), the generic path
    must be exact on all axes."""
    names = run_case(kom, kmp_opt, ROW_BY_ID[rid], Case(_own(ROW_BY_ID[rid]), region=region))
    assert names == {'encode': 'encode_generic', 'decode': 'decode_generic'}


@pytest.mark.parametrize('rid', [r[0] for r in LIN2D])
def test_lin2d_matches_the_two_pass_path(kom, kmp_opt, rid):
    """The image LinearPredictor cells computed inside the row kernel give the bytes of the two-pass
    path (KMP_DISABLE_LINEAR_FUSED=1), whole and for a row region."""
    from kompressor_amd import _nd, _lib
    row = ROW_BY_ID[rid]
    _, shape, dtype, _, p, *_ = row
    ns = kom.image
    ref = _reference(kom, kmp_opt, row, 'random')
    B = shape[0]
    x = torch.from_numpy(ref['x'][:B]).cuda()
    lo_in = torch.from_numpy(ref['lowres'][:B]).cuda()
    maps_in = [torch.from_numpy(m[:B]).cuda() for m in ref['maps']]
    pred = _predictor_for(kom, row, 'random')
    E = ref['lowres'].shape[1:3]
    penc = _nd.fused_plan(pred, getattr(ns, 'encode_values_' + CODER[dtype]), p, NP2T[dtype], 2, _lib.ENCODE)
    pdec = _nd.fused_plan(pred, getattr(ns, 'decode_values_' + CODER[dtype]), p, NP2T[dtype], 2, _lib.DECODE)
    for region in (None, [(1, E[0] - 1), (0, E[1])]):
        got = []
        for disable in (None, 1):
            kmp_opt('KMP_DISABLE_LINEAR_FUSED', disable)
            lo = _nd._zeros(lo_in.shape, lo_in.dtype)
            maps = [_nd._zeros(m.shape, m.dtype) for m in maps_in]
            _nd.fused_encode_into(x, penc[0], penc[1], lo, maps, 2, region=region)
            assert kom._lib.lib.kmp_last_launch().decode() == 'encode_generic'
            out = _nd._zeros(x.shape, x.dtype)
            _nd.fused_decode_into(lo_in, maps_in, ref['dims'], pdec[0], pdec[1], out, 2, region=region)
            assert kom._lib.lib.kmp_last_launch().decode() == 'decode_generic'
            got.append([t.cpu().numpy().tobytes() for t in (lo, *maps, out)])
        kmp_opt('KMP_DISABLE_LINEAR_FUSED', None)
        assert got[0] == got[1], f'{rid} region {region}'


@pytest.mark.parametrize('rid', ['vol-u16-p1', 'vol-lin-mfma-p1', 'img-u8-p0'])
def test_guard_reads_the_device_arenas(kom, kmp_opt, rid):
    """The checks see what the kernels wrote: a launch on z planes / rows [1, E - 1) judged by the masks
    of [1, E - 2) wrote one plane 'outside its box', in lowres and in every map that has that plane;
    judged by [0, E - 1) it left plane 0 unwritten."""
    row = ROW_BY_ID[rid]
    ndim = len(row[1]) - 2
    E = _reference(kom, kmp_opt, row, 'random')['lowres'].shape[1:1 + ndim]
    rest = [(0, int(e)) for e in E[1:]]
    with pytest.raises(G.GuardError) as e:
        run_case(kom, kmp_opt, row, Case(_own(row), 'inside', claim=[(1, E[0] - 2)] + rest))
    outputs = ['lowres'] + [f'map{k}' for k in range(7 if ndim == 3 else 3)]
    assert {(c, n) for c, n, _ in e.value.failures} == {('unowned', n) for n in outputs}
    with pytest.raises(G.GuardError) as e:
        run_case(kom, kmp_opt, row, Case(_own(row), 'inside', claim=[(0, E[0] - 1)] + rest))
    # the unwritten plane holds the sentinel: not the reference, and another byte in the second run
    assert {(c, n) for c, n, _ in e.value.failures} == \
        {(c, n) for c in ('value', 'nondeterministic') for n in outputs}


def test_every_family_was_reached():
    """Runs last: each launch name was reached in both directions with a region and B % 8 == 0 in
    one launch.  fast2d takes no region at all (f2::geometry, kmp_codec_fast2d.hip: ``|| region``), so
    for it the requirement is B % 8 == 0 on the whole frame, and a region on its rows is pinned to
    the generic path above."""
    assert SEEN, 'run the whole module: this test reads the launches the tests above collected'
    missing = []
    for fam in REQUIRED:
        for direction in ('encode', 'decode'):
            if (fam, direction, fam != 'fast2d', True) not in SEEN:
                missing.append((fam, direction))
    assert not missing, f'never launched with a region at B % 8 == 0: {missing}'
    assert not any(proper for fam, _, proper, _ in SEEN if fam == 'fast2d')
