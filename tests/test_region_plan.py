"""container.plan_region / container.info: the host logic of partial reads, on the CPU.

The plan says which planes of which array a selection needs.  Its sufficiency is checked against
the numpy oracle: a pyramid is encoded with ``oracle.volume.encode``, every level's local arrays are
built from ONLY what the plan selects (a poison value everywhere else), decoded with
``oracle.volume.decode`` from the coarsest level up, cropped, and compared with the input."""

import json
import struct

import numpy as np
import pytest

import oracle
from oracle import predictors as OP
from oracle import rice as R
from kompressor_amd import container, _nd

POISON = 0xBEEF


def _meta(shape, levels, p):
    """The metadata ``compress`` records for a ``levels``-deep pyramid of ``shape``."""
    lv, s = [], tuple(shape)
    for _ in range(levels):
        lo, _, dims = _nd.encoded_shapes(s, 3)
        lv.append({'highres_shape': list(s), 'dims': [int(d) for d in dims]})
        s = tuple(lo)
    return {'format': 'kompressor_amd', 'ndim': 3, 'padding': p, 'method': 'rice', 'sample_dtype': 'uint16',
            'levels': lv, 'lowres_shape': list(s), 'predictor': {'kind': 'mean', 'padding': p, 'ndim': 3}}


def test_known_answer():
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
    # level 0: planes [9, 11) land at local plane 9 - 7; the local lowres has 6 planes and is not at the
    # top, so a map that is odd along z (map 0) has 6 - 1 local planes and an even one (map 2) has 6
    m = plan['arrays'][1]
    assert m['shape'] == (1, 20, 64, 64, 1) and m['local_shape'] == (1, 5, 64, 64, 1) and m['local_at'] == 2
    assert m['ranges'] == [(9 * 4096, 11 * 4096, 2 * 4096)]
    assert plan['arrays'][3]['local_shape'] == (1, 6, 64, 64, 1)


def test_full_selection_clamping_and_errors():
    meta = _meta((3, 33, 20, 24, 1), 3, 2)
    for kw in ({}, {'planes': (0, 33), 'batch': (0, 3)}, {'planes': (-5, 99), 'batch': (-1, 7)}):
        plan = container.plan_region(meta, **kw)
        assert plan['tiles_decoded'] == plan['tiles_total'] and len(plan['arrays']) == 1 + 3 * 7
        for ar in plan['arrays']:
            assert ar['ranges'] == [(0, int(np.prod(ar['shape'])), 0)] and ar['local_shape'] == ar['shape']
        assert all(lv['at_top'] for lv in plan['levels'])
    plan = container.plan_region(meta, planes=(30, 99), batch=(2, 9))
    assert plan['planes'] == (30, 33) and plan['batch'] == (2, 3)
    # a batch range alone is one contiguous range per array; with planes, one per batch item
    plan = container.plan_region(meta, batch=(1, 3))
    assert all(len(ar['ranges']) == 1 and ar['ranges'][0][0] == int(np.prod(ar['shape'][1:])) for ar in plan['arrays'])
    plan = container.plan_region(meta, batch=(1, 3), planes=(4, 9))
    assert all(len(ar['ranges']) == 2 for ar in plan['arrays'][1:8])   # the finest level's maps
    assert all(len(ar['ranges']) == (1 if ar['sel'] == (0, ar['shape'][1]) else 2) for ar in plan['arrays'])
    for kw in ({'planes': (5, 5)}, {'planes': (9, 4)}, {'planes': (33, 40)}, {'batch': (3, 4)}, {'batch': (2, 1)}):
        with pytest.raises(ValueError):
            container.plan_region(meta, **kw)
    image = {'ndim': 2, 'padding': 0, 'levels': [{'highres_shape': [6, 40, 48, 1], 'dims': [1, 1]}],
             'lowres_shape': [6, 20, 24, 1]}
    with pytest.raises(ValueError):
        container.plan_region(image, planes=(0, 4))
    assert [ar['ranges'] for ar in container.plan_region(image, batch=(2, 5))['arrays']] == \
        [[(2 * 480, 5 * 480, 0)]] * 4


_PYRAMIDS = {}


def _pyramid(D, p, levels):
    """``(volume, coarsest lowres, per level (maps, dims))`` by the numpy oracle, computed once."""
    key = (D, p, levels)
    if key not in _PYRAMIDS:
        rng = np.random.default_rng(D * 10 + p)
        vol = rng.integers(0, 65536, (1, D, 9, 10, 1), dtype=np.int64).astype(np.uint16)
        fn = OP.mean_predictions_fn(p, 3)
        x, per = vol, []
        for _ in range(levels):
            x, (maps, dims) = oracle.volume.encode(fn, oracle.volume.encode_values_uint16, x, padding=p)
            per.append(([np.asarray(m) for m in maps], tuple(int(d) for d in dims)))
        _PYRAMIDS[key] = (vol, np.asarray(x), per)
    return _PYRAMIDS[key]


def _cases():
    for D in (7, 8, 21, 33, 34):
        auto = container._auto_levels((1, D, 9, 10, 1), 3)
        for levels in (1, 2, 3):
            if levels > auto:  # deeper than compress(levels='auto') makes them
                continue
            for p in (0, 1, 2):
                for planes in ((0, 1), (0, D), (D - 1, D), (D // 2, D // 2 + 1), (1, 2), (3, 6), (2, 7)):
                    yield D, p, levels, planes


CASES = list(_cases())


def test_case_grid_size():
    assert len(CASES) == 273


@pytest.mark.parametrize('D,p,levels,planes', CASES)
def test_plan_is_sufficient_against_the_oracle(D, p, levels, planes):
    vol, coarsest, per = _pyramid(D, p, levels)
    plan = container.plan_region(_meta(vol.shape, levels, p), planes=planes)
    fn = OP.mean_predictions_fn(p, 3)
    lo, hi = plan['lowres']
    x = coarsest[:, lo:hi]
    assert plan['arrays'][0]['local_shape'] == x.shape
    for lvl in reversed(range(levels)):
        L = plan['levels'][lvl]
        maps, dims = per[lvl]
        local = []
        for k, m in enumerate(maps):
            ar = plan['arrays'][1 + 7 * lvl + k]
            assert ar['shape'] == m.shape and ar['sel'] == L['maps'][k]
            s0, s1 = ar['sel']
            buf = np.full(ar['local_shape'], POISON, m.dtype)
            buf[:, ar['local_at']:ar['local_at'] + s1 - s0] = m[:, s0:s1]
            local.append(buf)
        ldims = (dims[0] if L['at_top'] else 0, dims[1], dims[2])
        out = np.asarray(oracle.volume.decode(fn, oracle.volume.decode_values_uint16, x, (local, ldims), padding=p))
        a, b = L['highres']
        x = out[:, a - 2 * L['lowres'][0]:b - 2 * L['lowres'][0]]
    assert np.array_equal(x, vol[:, planes[0]:planes[1]])


def test_info_reads_header_and_metadata_only(tmp_path):
    vol, coarsest, per = _pyramid(21, 1, 2)
    bundle = R.pack_bundle([coarsest] + [m for maps, _ in per for m in maps]).tobytes()
    meta = dict(_meta(vol.shape, 2, 1), bundle_bytes=len(bundle), crc32=0)
    js = json.dumps(meta).encode()
    js += b' ' * (-len(js) % 8)
    path = tmp_path / 'hand.kmp'
    path.write_bytes(struct.pack('<4sHHQ', b'KMPF', 3, 0, len(js)) + js + bundle)
    got = container.info(str(path))
    assert got == {'shape': (1, 21, 9, 10, 1), 'sample_dtype': 'uint16', 'ndim': 3, 'levels': 2, 'padding': 1,
                   'predictor': 'mean', 'method': 'rice', 'version': 3, 'file_bytes': 16 + len(js) + len(bundle),
                   'bundle_bytes': len(bundle)}
    (tmp_path / 'short.kmp').write_bytes(path.read_bytes()[:-1])
    with pytest.raises(ValueError):
        container.info(str(tmp_path / 'short.kmp'))
    with pytest.raises(ValueError):
        (tmp_path / 'junk.kmp').write_bytes(b'GIF89a' + bytes(64))
        container.info(str(tmp_path / 'junk.kmp'))
