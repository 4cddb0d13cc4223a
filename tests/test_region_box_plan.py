"""container.plan_region with rows, cols and level / container.level_shapes: the host logic of box
and level reads, on the CPU.

Known answers, by hand.  File ``[1, 40, 128, 128, 1]``, 2 levels, padding 1, selection
``planes=(18, 22), rows=(40, 60), cols=(5, 9)``, the row-crop threshold patched to 1 so rows are
cropped at every level:

  level 0 (lowres 20 x 64 x 64, every map ``(1, 20, 64, 64, 1)``)
    planes (18, 22) -> out (9, 11)  -> lowres (9 - 2, 11 + 2) = (7, 13)     6 local planes, not at the top
    rows   (40, 60) -> out (20, 30) -> lowres (18, 32)                      14 local rows, not at the top
    cols   (5, 9)   -> out (2, 5)   -> lowres (0, 7); the local arrays keep all 64 columns (at the top)
    a map odd along z and y (map 0) is local (1, 5, 13, 64, 1), one even along both (map 6) (1, 6, 14, 64, 1);
    the selection starts at local plane 9 - 7 = 2 and local row 20 - 18 = 2; one row run per plane:
    plane 9: samples (9 * 64 + 20) * 64 = 38144 .. (9 * 64 + 30) * 64 = 38784 to (2 * 13 + 2) * 64 = 1792 (map 0),
    plane 10: 42240 .. 42880 to (3 * 13 + 2) * 64 = 2624; both inside tile 2: 2 tiles per map, 14 in all
  level 1 (lowres 10 x 32 x 32, every map ``(1, 10, 32, 32, 1)``, 10240 samples: one tile)
    planes (7, 13)  -> out (3, 7)   -> lowres (1, 9)      rows (18, 32) -> out (9, 16) -> lowres (7, 18)
    cols   (0, 7)   -> out (0, 4)   -> lowres (0, 6)
    map 0 is local (1, 7, 10, 32, 1); 4 row runs per map, plane 3: (3 * 32 + 9) * 32 = 3360 .. 3584: 28 tiles
  coarsest lowres ``(1, 10, 32, 32, 1)``: planes (1, 9), rows (7, 18): local (1, 8, 11, 32, 1), 8 row runs,
    plane 1: (32 + 7) * 32 = 1248 .. (32 + 18) * 32 = 1600 to 0: 8 tiles
  tiles_decoded = 14 + 28 + 8 = 50 of the file's 43: the one-tile planes are decoded again per run,
  which is what the threshold prevents -- at the default threshold level 0's plane of cells is
  64 * 64 = 4096 <= 16384 samples, rows are not cropped anywhere and the plan is the planes-only plan
  (15 tiles) with the column spans added.

Sufficiency is checked against the numpy oracle as in test_region_plan.py: the local arrays are
filled through the plan's ``ranges`` alone (a poison value everywhere else, unselected rows
included), decoded with the oracle from the coarsest level up to the level asked for, cropped, and
compared with the strided input."""

import json
import struct

import numpy as np
import pytest

import oracle
from oracle import predictors as OP
from oracle import rice as R
from kompressor_amd import container, _nd

POISON = 0xBEEF


def _meta(shape, levels, p, ndim=3):
    lv, s = [], tuple(shape)
    for _ in range(levels):
        lo, _, dims = _nd.encoded_shapes(s, ndim)
        lv.append({'highres_shape': list(s), 'dims': [int(d) for d in dims]})
        s = tuple(lo)
    return {'format': 'kompressor_amd', 'ndim': ndim, 'padding': p, 'method': 'rice', 'sample_dtype': 'uint16',
            'levels': lv, 'lowres_shape': list(s), 'predictor': {'kind': 'mean', 'padding': p, 'ndim': ndim}}


@pytest.fixture
def crop_everywhere(monkeypatch):
    monkeypatch.setattr(container, '_ROW_CROP_PLANE', 1)


KNOWN = dict(planes=(18, 22), rows=(40, 60), cols=(5, 9))


def test_known_answer_rows_cropped(crop_everywhere):
    plan = container.plan_region(_meta((1, 40, 128, 128, 1), 2, 1), **KNOWN)
    assert (plan['planes'], plan['rows'], plan['cols'], plan['level']) == ((18, 22), (40, 60), (5, 9), 0)
    l0, l1 = plan['levels']
    assert (l0['highres'], l0['out'], l0['lowres'], l0['at_top']) == ((18, 22), (9, 11), (7, 13), False)
    assert (l0['rows']['highres'], l0['rows']['out'], l0['rows']['lowres'], l0['rows']['local']) == \
        ((40, 60), (20, 30), (18, 32), (18, 32))
    assert (l0['cols']['highres'], l0['cols']['out'], l0['cols']['lowres'], l0['cols']['local']) == \
        ((5, 9), (2, 5), (0, 7), (0, 64))
    assert l0['at_top_axes'] == (False, False, True)
    assert [A['crop'] for A in l0['axes']] == [(18 - 14, 22 - 14), (40 - 36, 60 - 36), (5, 9)]
    assert (l1['highres'], l1['out'], l1['lowres']) == ((7, 13), (3, 7), (1, 9))
    assert (l1['rows']['highres'], l1['rows']['out'], l1['rows']['lowres']) == ((18, 32), (9, 16), (7, 18))
    assert (l1['cols']['highres'], l1['cols']['out'], l1['cols']['lowres']) == ((0, 7), (0, 4), (0, 6))
    assert l1['at_top_axes'] == (False, False, True)
    assert [A['crop'] for A in l1['axes']] == [(7 - 2, 13 - 2), (18 - 14, 32 - 14), (0, 64)]
    assert plan['lowres'] == (1, 9) and plan['lowres_axes'] == [(1, 9), (7, 18), (0, 32)]
    ar = plan['arrays']
    assert len(ar) == 15
    m = ar[1]  # level 0, odd along z and y
    assert m['shape'] == (1, 20, 64, 64, 1) and m['local_shape'] == (1, 5, 13, 64, 1)
    assert (m['sel'], m['local_at'], m['sel_rows'], m['local_row_at']) == ((9, 11), 2, (20, 30), 2)
    assert m['ranges'] == [(38144, 38784, 1792), (42240, 42880, 2624)]
    assert ar[7]['local_shape'] == (1, 6, 14, 64, 1)  # even along z and y
    assert ar[7]['ranges'] == [(38144, 38784, (2 * 14 + 2) * 64), (42240, 42880, (3 * 14 + 2) * 64)]
    m = ar[8]   # level 1, odd along z and y
    assert m['shape'] == (1, 10, 32, 32, 1) and m['local_shape'] == (1, 7, 10, 32, 1)
    assert m['ranges'] == [((z * 32 + 9) * 32, (z * 32 + 16) * 32, ((2 + z - 3) * 10 + 2) * 32) for z in range(3, 7)]
    assert m['ranges'][0][:2] == (3360, 3584)
    lo = ar[0]
    assert lo['shape'] == (1, 10, 32, 32, 1) and lo['local_shape'] == (1, 8, 11, 32, 1)
    assert lo['ranges'] == [((z * 32 + 7) * 32, (z * 32 + 18) * 32, (z - 1) * 11 * 32) for z in range(1, 9)]
    assert lo['ranges'][0] == (1248, 1600, 0)
    per = lambda arrays: sum((e - 1) // 16384 - f // 16384 + 1 for a in arrays for f, e, _ in a['ranges'])
    assert (per(ar[1:8]), per(ar[8:15]), per(ar[:1])) == (14, 28, 8)
    assert (plan['tiles_decoded'], plan['tiles_total']) == (50, 43)


def _strip(level):
    return {k: v for k, v in level.items() if k in ('highres', 'out', 'lowres', 'maps', 'at_top', 'dims')}


def test_known_answer_default_threshold():
    """Level 0's plane of cells is 64 * 64 <= one tile: rows are cropped nowhere, and the plan is the
    planes-only plan with the column spans added."""
    meta = _meta((1, 40, 128, 128, 1), 2, 1)
    plan = container.plan_region(meta, **KNOWN)
    base = container.plan_region(meta, planes=(18, 22))
    assert plan['arrays'] == base['arrays'] and plan['lowres'] == base['lowres']
    assert (plan['tiles_decoded'], plan['tiles_total']) == (15, 43)
    assert [_strip(lv) for lv in plan['levels']] == [_strip(lv) for lv in base['levels']]
    for lv, S in zip(plan['levels'], (128, 64)):
        assert lv['rows']['highres'] == (0, S) and lv['rows']['local'] == (0, S // 2)
        assert lv['at_top_axes'] == (False, True, True)
    assert [lv['cols']['out'] for lv in plan['levels']] == [(2, 5), (0, 4)]
    assert [lv['cols']['out'] for lv in base['levels']] == [(0, 64), (0, 32)]
    assert plan['levels'][0]['rows']['crop'] == (40, 60) and plan['levels'][0]['cols']['crop'] == (5, 9)
    assert (plan['rows'], plan['cols']) == ((40, 60), (5, 9)) and (base['rows'], base['cols']) == ((0, 128), (0, 128))


def test_known_answer_levels(crop_everywhere):
    meta = _meta((1, 40, 128, 128, 1), 2, 1)
    # level 1 is the (1, 20, 64, 64, 1) array: the finest level's maps are not read
    plan = container.plan_region(meta, planes=(7, 13), rows=(18, 32), cols=(0, 7), level=1)
    assert plan['level'] == 1 and [lv['index'] for lv in plan['levels']] == [1]
    assert all(ar['ranges'] == [] and ar['local_shape'] is None for ar in plan['arrays'][1:8])
    assert all(ar['ranges'] for ar in plan['arrays'][8:]) and plan['arrays'][0]['ranges']
    # the same spans as level 1 of the level-0 read above, which asked for exactly this box of it
    full = container.plan_region(meta, **KNOWN)
    assert plan['arrays'][8:] == full['arrays'][8:] and plan['arrays'][0] == full['arrays'][0]
    assert plan['tiles_decoded'] == 28 + 8 and plan['tiles_total'] == 43
    # level 2 is the stored coarsest lowres: no map is read, no level is decoded
    plan = container.plan_region(meta, planes=(1, 9), rows=(7, 18), cols=(3, 5), level=2)
    assert plan['levels'] == [] and plan['box'] == ((1, 9), (7, 18), (3, 5))
    assert all(ar['ranges'] == [] for ar in plan['arrays'][1:])
    assert plan['arrays'][0] == full['arrays'][0] and plan['tiles_decoded'] == 8
    whole = container.plan_region(meta, level=2)
    assert whole['arrays'][0]['ranges'] == [(0, 10240, 0)] and whole['tiles_decoded'] == 1


def test_no_new_keyword_plan_is_the_parents():
    """What test_region_plan.test_known_answer pins, on a call without the new keywords."""
    plan = container.plan_region(_meta((1, 40, 128, 128, 1), 2, 1), planes=(18, 22))
    l0, l1 = plan['levels']
    assert (l0['out'], l0['lowres']) == ((9, 11), (7, 13))
    assert (l1['highres'], l1['out'], l1['lowres']) == ((7, 13), (3, 7), (1, 9))
    assert plan['lowres'] == (1, 9) and plan['planes'] == (18, 22) and plan['batch'] == (0, 1)
    assert not l0['at_top'] and not l1['at_top']
    assert l0['maps'] == [(9, 11)] * 7 and l1['maps'] == [(3, 7)] * 7
    assert (plan['tiles_decoded'], plan['tiles_total']) == (15, 43)
    lowres = plan['arrays'][0]
    assert lowres['shape'] == (1, 10, 32, 32, 1) and lowres['local_shape'] == (1, 8, 32, 32, 1)
    assert lowres['ranges'] == [(1 * 1024, 9 * 1024, 0)]
    m = plan['arrays'][1]
    assert m['shape'] == (1, 20, 64, 64, 1) and m['local_shape'] == (1, 5, 64, 64, 1) and m['local_at'] == 2
    assert m['ranges'] == [(9 * 4096, 11 * 4096, 2 * 4096)]
    assert plan['arrays'][3]['local_shape'] == (1, 6, 64, 64, 1)
    assert plan['level'] == 0 and (plan['rows'], plan['cols']) == ((0, 128), (0, 128))


def test_clamping_and_errors(crop_everywhere):
    meta = _meta((3, 33, 20, 24, 1), 3, 2)
    plan = container.plan_region(meta, planes=(-5, 99), rows=(-3, 50), cols=(-1, 24), batch=(-1, 7))
    assert plan['box'] == ((0, 33), (0, 20), (0, 24)) and plan['batch'] == (0, 3)
    assert plan['tiles_decoded'] == plan['tiles_total']
    for ar in plan['arrays']:
        assert ar['ranges'] == [(0, int(np.prod(ar['shape'])), 0)] and ar['local_shape'] == ar['shape']
    plan = container.plan_region(meta, rows=(17, 99), cols=(20, 99))
    assert (plan['rows'], plan['cols']) == ((17, 20), (20, 24))
    # level 1 of 33 x 20 x 24 is 17 x 10 x 12: the ranges clamp to it
    plan = container.plan_region(meta, planes=(10, 99), rows=(8, 99), cols=(0, 99), level=1)
    assert plan['box'] == ((10, 17), (8, 10), (0, 12))
    assert container.plan_region(meta, level=3)['arrays'][0]['local_shape'] == (3, 5, 3, 3, 1)
    bad = [{'rows': (5, 5)}, {'rows': (9, 4)}, {'rows': (20, 30)}, {'cols': (7, 7)}, {'cols': (8, 2)}, {'cols': (24, 25)},
           {'planes': (5, 5)}, {'level': -1}, {'level': 4}, {'level': 1.5}, {'level': None}, {'level': True},
           {'level': 1, 'planes': (17, 20)}, {'level': 1, 'rows': (10, 12)}, {'level': 3, 'cols': (3, 4)}]
    for kw in bad:
        with pytest.raises(ValueError):
            container.plan_region(meta, **kw)


def test_image_takes_rows_and_cols_and_refuses_planes():
    image = {'ndim': 2, 'padding': 0, 'levels': [{'highres_shape': [6, 40, 48, 1], 'dims': [1, 1]}],
             'lowres_shape': [6, 20, 24, 1]}
    for kw in ({'planes': (0, 4)}, {'planes': (0, 4), 'rows': (0, 4)}, {'planes': (0, 4), 'level': 1}):
        with pytest.raises(ValueError):
            container.plan_region(image, **kw)
    plan = container.plan_region(image, rows=(10, 14), cols=(7, 9), batch=(2, 4))
    (lv,) = plan['levels']
    # rows are an image's first spatial axis: the keys that meant z for a volume describe them
    assert lv['rows'] is lv['axes'][0] and (lv['highres'], lv['out'], lv['lowres']) == ((10, 14), (5, 7), (4, 8))
    assert (lv['cols']['out'], lv['cols']['lowres'], lv['cols']['local']) == ((3, 5), (2, 6), (0, 24))
    assert plan['arrays'][0]['local_shape'] == (2, 4, 24, 1)
    assert plan['arrays'][0]['ranges'] == [((b * 20 + 4) * 24, (b * 20 + 8) * 24, (b - 2) * 4 * 24) for b in (2, 3)]
    assert plan['arrays'][1]['local_shape'] == (2, 3, 24, 1)   # odd along y: 4 - 1 local rows
    assert plan['arrays'][1]['ranges'] == [((b * 20 + 5) * 24, (b * 20 + 7) * 24, ((b - 2) * 3 + 1) * 24) for b in (2, 3)]
    plan = container.plan_region(image, rows=(3, 9), level=1)
    assert plan['levels'] == [] and plan['arrays'][0]['ranges'] == [(b * 480 + 72, b * 480 + 216, (b * 6) * 24)
                                                                    for b in range(6)]
    with pytest.raises(ValueError):
        container.plan_region(image, level=2)


# ---------------------------------------------------------------------------------------------
# sufficiency against the numpy oracle
# ---------------------------------------------------------------------------------------------

_PYRAMIDS = {}


def _pyramid(shape, p, levels):
    """``(array, per level k the array of level k, coarsest lowres, per level (maps, dims))`` by the
    numpy oracle, computed once."""
    key = (shape, p, levels)
    if key not in _PYRAMIDS:
        ndim = len(shape) - 2
        mod = oracle.volume if ndim == 3 else oracle.image
        rng = np.random.default_rng(sum(shape) * 10 + p)
        vol = rng.integers(0, 65536, shape, dtype=np.int64).astype(np.uint16)
        fn = OP.mean_predictions_fn(p, ndim)
        x, per, tops = vol, [], []
        for _ in range(levels):
            tops.append(x)
            x, (maps, dims) = mod.encode(fn, oracle.volume.encode_values_uint16, x, padding=p)
            x = np.asarray(x)
            per.append(([np.asarray(m) for m in maps], tuple(int(d) for d in dims)))
        tops.append(x)
        _PYRAMIDS[key] = (vol, tops, x, per)
    return _PYRAMIDS[key]


def _fill(ar, src):
    """The local array of plan entry ``ar``, filled through its ranges alone."""
    buf = np.full(ar['local_shape'], POISON, src.dtype)
    flat, s = buf.reshape(-1), src.reshape(-1)
    for first, end, dst in ar['ranges']:
        assert 0 <= first < end <= s.size and 0 <= dst and dst + end - first <= flat.size
        flat[dst:dst + end - first] = s[first:end]
    return buf


def _decode_by_plan(shape, p, levels, kw):
    ndim = len(shape) - 2
    mod = oracle.volume if ndim == 3 else oracle.image
    vol, tops, coarsest, per = _pyramid(shape, p, levels)
    plan = container.plan_region(_meta(shape, levels, p, ndim), **kw)
    fn = OP.mean_predictions_fn(p, ndim)
    nmaps = len(_nd.PARITY[ndim])
    x = _fill(plan['arrays'][0], coarsest)
    assert not (x == POISON).all()
    for L in reversed(plan['levels']):
        lvl = L['index']
        maps, dims = per[lvl]
        local = []
        for k, m in enumerate(maps):
            ar = plan['arrays'][1 + nmaps * lvl + k]
            assert ar['shape'] == m.shape
            local.append(_fill(ar, m))
        ldims = tuple(d if top else 0 for d, top in zip(dims, L['at_top_axes']))
        out = np.asarray(mod.decode(fn, oracle.volume.decode_values_uint16, x, (local, ldims), padding=p))
        x = out[(slice(None), *[slice(*A['crop']) for A in L['axes']])]
    if not plan['levels']:
        x = x[(slice(None), *[slice(s - lo, e - lo) for (s, e), (lo, _) in zip(plan['box'], plan['lowres_axes'])])]
    k = plan['level']
    assert vol[(slice(None), *[slice(None, None, 2 ** k)] * ndim)].shape == tops[k].shape
    assert np.array_equal(vol[(slice(None), *[slice(None, None, 2 ** k)] * ndim)], tops[k])
    b0, b1 = plan['batch']
    want = tops[k][(slice(b0, b1), *[slice(s, e) for s, e in plan['box']])]
    return x, want, plan


def _spans(n):
    """The first, the last, one interior, a span crossing the middle, the whole axis."""
    return [(0, 1), (n - 1, n), (n // 3, n // 3 + 1), (n // 2 - 1, n // 2 + 2), (0, n)]


def _cases():
    for D, H, W in ((7, 8, 9), (8, 13, 10), (21, 12, 11)):
        shape = (1, D, H, W, 1)
        auto = container._auto_levels(shape, 3)
        for levels in (1, 2, 3):
            if levels > auto:
                continue
            for p in (0, 1, 2):
                for level in (0, 1):
                    ext = [-(-s // 2 ** level) for s in (D, H, W)]
                    for rows in _spans(ext[1]):
                        for planes in ((0, 1), (ext[0] // 2, ext[0])):
                            for cols in ((ext[2] - 1, ext[2]), (1, ext[2] // 2 + 1)):
                                yield shape, p, levels, level, planes, rows, cols


CASES = list(_cases())


def test_box_case_grid_size():
    # 3 volumes of (2, 2, 3) level counts (what _auto_levels allows), 3 paddings, 2 levels to read, 5 x 2 x 2 boxes
    assert len(CASES) == (2 + 2 + 3) * 3 * 2 * 20 == 840


@pytest.mark.parametrize('shape,p,levels,level,planes,rows,cols', CASES)
def test_box_plan_is_sufficient_against_the_oracle(crop_everywhere, shape, p, levels, level, planes, rows, cols):
    got, want, plan = _decode_by_plan(shape, p, levels, dict(planes=planes, rows=rows, cols=cols, level=level))
    assert want.size and np.array_equal(got, want)
    for ar in plan['arrays']:  # a row-cropped array is read as one row run per selected plane, else as one range
        if ar['local_shape'] is not None and ar['ranges']:
            cropped = ar['local_shape'][2] != ar['shape'][2] or ar['sel_rows'] != (0, ar['shape'][2])
            assert len(ar['ranges']) == (ar['sel'][1] - ar['sel'][0] if cropped else 1)


def _row_cropped(plan):
    return any(ar['local_shape'] is not None and ar['local_shape'][2] != ar['shape'][2] for ar in plan['arrays'])


def test_the_grid_crops_rows(monkeypatch):
    def plans():
        return [container.plan_region(_meta(shape, levels, p), planes=planes, rows=rows, cols=cols, level=level)
                for shape, p, levels, level, planes, rows, cols in CASES]
    assert not any(_row_cropped(pl) for pl in plans())  # planes this small: never at the default threshold
    monkeypatch.setattr(container, '_ROW_CROP_PLANE', 1)
    # every extent has >= 4 cells along y: at p = 0 the first row needs cells (0, 2) and the last one at most 2 more
    for case, pl in zip(CASES, plans()):
        shape, p, levels, level, planes, rows, cols = case
        if p == 0 and level == 0 and rows in ((0, 1), (shape[2] - 1, shape[2])):
            assert _row_cropped(pl), case


def test_default_threshold_is_sufficient_too():
    for rows in _spans(12):
        got, want, plan = _decode_by_plan((1, 21, 12, 11, 1), 1, 3, dict(planes=(5, 9), rows=rows, cols=(2, 7)))
        assert np.array_equal(got, want)
        assert all(len(ar['ranges']) == 1 for ar in plan['arrays'])  # planes this small are never row-cropped


IMAGE_CASES = [(p, levels, level, rows, cols) for p in (0, 1, 2) for levels in (1, 2) for level in (0, 1)
               for rows in _spans(-(-13 // 2 ** level)) for cols in ((0, 1), (2, 5), (0, -(-12 // 2 ** level)))]


@pytest.mark.parametrize('p,levels,level,rows,cols', IMAGE_CASES)
def test_image_plan_is_sufficient_against_the_oracle(p, levels, level, rows, cols):
    assert len(IMAGE_CASES) == 180
    for batch in (None, (1, 2)):
        got, want, _ = _decode_by_plan((2, 13, 12, 1), p, levels, dict(rows=rows, cols=cols, level=level, batch=batch))
        assert want.size and np.array_equal(got, want)


# ---------------------------------------------------------------------------------------------
# level_shapes
# ---------------------------------------------------------------------------------------------

def test_level_shapes_reads_header_and_metadata_only(tmp_path):
    vol, tops, coarsest, per = _pyramid((1, 21, 12, 11, 1), 1, 2)
    bundle = R.pack_bundle([coarsest] + [m for maps, _ in per for m in maps]).tobytes()
    meta = dict(_meta(vol.shape, 2, 1), bundle_bytes=len(bundle), crc32=0)
    js = json.dumps(meta).encode()
    js += b' ' * (-len(js) % 8)
    path = tmp_path / 'hand.kmp'
    path.write_bytes(struct.pack('<4sHHQ', b'KMPF', 3, 0, len(js)) + js + bundle)
    got = container.level_shapes(str(path))
    assert got == [(1, 21, 12, 11, 1), (1, 11, 6, 6, 1), (1, 6, 3, 3, 1)]
    assert got == [t.shape for t in tops] and got[0] == container.info(str(path))['shape']
    assert got == [vol[:, ::s, ::s, ::s].shape for s in (1, 2, 4)]
    (tmp_path / 'short.kmp').write_bytes(path.read_bytes()[:-1])
    with pytest.raises(ValueError):
        container.level_shapes(str(tmp_path / 'short.kmp'))
    (tmp_path / 'junk.kmp').write_bytes(b'GIF89a' + bytes(64))
    with pytest.raises(ValueError):
        container.level_shapes(str(tmp_path / 'junk.kmp'))
    broken = dict(meta, levels=[{'dims': [0, 1, 0]}])
    js = json.dumps(broken).encode()
    js += b' ' * (-len(js) % 8)
    (tmp_path / 'nometa.kmp').write_bytes(struct.pack('<4sHHQ', b'KMPF', 3, 0, len(js)) + js + bundle)
    with pytest.raises(ValueError):
        container.level_shapes(str(tmp_path / 'nometa.kmp'))
