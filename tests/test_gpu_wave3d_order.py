"""The metric kernel's decode order and encode tail policy (kmp_codec_wave3d.hip): KMP_W3_DEC_REV
walks the decode's blocks last-first, KMP_W3_ST_TAIL (KiB) stores the tail of the encode's output
(at most half of the call's blocks) with the default cache policy.  Neither may change a byte: every setting gives the oracle's lowres
and maps and a lossless decode, on the smallest shapes that reach each branch of the kernel."""

import itertools

import numpy as np
import pytest
import torch

from conftest import load_golden, golden_maps

pytestmark = pytest.mark.gpu

# (shape, dtype, tails in KiB: none, one block's worth, about half the batch, more than the batch)
SHAPES = {
    # C3 tile, B % 8 == 0: the XCD order is active; 128 blocks of 32 KiB (PL = 2), 4 MiB in all
    'tile64x8': ((8, 64, 64, 64, 1), np.uint16, (0, 32, 2048, 8192)),
    # identity order, 48 blocks: nvblk - 1 - vblk is not congruent to vblk mod 8; 1.5 MiB
    'tile64x3': ((3, 64, 64, 64, 1), np.uint16, (0, 32, 768, 4096)),
    # u8, 8 outputs per lane: 32 blocks of 2 KiB
    'u8': ((16, 8, 16, 32, 1), np.uint8, (0, 2, 32, 128)),
    # 64 lanes per row, the one-row variant: 2 blocks (2 planes + 1 plane), 48 KiB
    'one_row': ((1, 6, 8, 512, 1), np.uint16, (0, 16, 32, 64)),
    # odd depth, a short last plane block, rows past Ey: 18 blocks of about 2.5 KiB
    'odd': ((9, 7, 10, 32, 1), np.uint16, (0, 3, 22, 64)),
}
CASES = [(n, None) for n in SHAPES] + [('tile64x8', 1), ('tile64x3', 1)]
GOLDEN_TILE = 5  # the tile of 'tile64x8' that holds the vol_tile64_p0 fixture's volume

_REF = {}


def _reference(name):
    """(highres, oracle lowres, oracle maps, dims) of a shape: computed once, never modified."""
    if name not in _REF:
        import oracle
        from oracle import predictors as OP
        shape, dtype, _ = SHAPES[name]
        x = np.random.default_rng(31).integers(0, np.iinfo(dtype).max + 1, size=shape, dtype=np.int64).astype(dtype)
        if name == 'tile64x8':
            x[GOLDEN_TILE] = load_golden('vol_tile64_p0')['highres'][0]
        oenc = oracle.volume.encode_values_uint16 if dtype == np.uint16 else oracle.volume.encode_values_uint8
        lo, (maps, dims) = oracle.volume.encode(OP.mean_predictions_fn(0, 3), oenc, x)
        for a in (x, lo, *maps):
            a.setflags(write=False)
        _REF[name] = (x, lo, tuple(maps), tuple(int(d) for d in dims))
    return _REF[name]


def _coders(kom, dtype):
    ns = kom.volume
    return (ns.encode_values_uint16, ns.decode_values_uint16) if dtype == np.uint16 else \
        (ns.encode_values_uint8, ns.decode_values_uint8)


def _last(kom):
    return kom._lib.lib.kmp_last_launch().decode()


@pytest.mark.parametrize('name,pl', CASES, ids=[f'{n}-pl{p or "dflt"}' for n, p in CASES])
def test_order_and_tail_are_output_neutral(kom, kmp_opt, name, pl):
    shape, dtype, tails = SHAPES[name]
    x, want_lo, want_maps, want_dims = _reference(name)
    enc, dec = _coders(kom, dtype)
    pred = kom.MeanPredictor(0, 3)
    xd = torch.from_numpy(x.copy()).cuda()
    if pl is not None:
        kmp_opt('KMP_W3_PL', pl)
    for rev, tail in itertools.product((0, 1), tails):
        kmp_opt('KMP_W3_DEC_REV', rev)
        kmp_opt('KMP_W3_ST_TAIL', tail)
        lo, (maps, dims) = kom.volume.encode(pred, enc, xd)
        assert _last(kom) == 'wave3d_encode', (rev, tail)
        assert tuple(int(d) for d in dims) == want_dims
        # every setting equals the oracle, so all settings give identical bytes
        assert np.array_equal(lo.cpu().numpy(), want_lo), (rev, tail)
        for k, (a, b) in enumerate(zip(maps, want_maps)):
            bad = np.argwhere(a.cpu().numpy() != b)
            assert bad.size == 0, f'rev={rev} tail={tail} map {k}: {len(bad)} mismatches, first at {bad[:3].tolist()}'
        rec = kom.volume.decode(pred, dec, lo, (maps, dims))
        assert _last(kom) == 'wave3d_decode', (rev, tail)
        assert torch.equal(rec, xd), (rev, tail)
    if name == 'tile64x8':
        g = load_golden('vol_tile64_p0')
        assert np.array_equal(lo[GOLDEN_TILE].cpu().numpy(), g['lowres'][0])
        for a, b in zip(maps, golden_maps(g, 3)):
            assert np.array_equal(a[GOLDEN_TILE].cpu().numpy(), b[0])


def test_z_region_inside_the_tile(kom, kmp_opt):
    """Encode and decode of a z-region that starts and ends inside the tile: the region's planes
    equal those of the full call, and nothing outside them is written, for every setting."""
    from kompressor_amd import _nd
    name = 'tile64x8'
    x, want_lo, want_maps, dims = _reference(name)
    pred = kom.MeanPredictor(0, 3)
    coder = _nd.NATURAL_CODER[torch.uint16]
    xd = torch.from_numpy(x.copy()).cuda()
    lo_full = torch.from_numpy(want_lo.copy()).cuda()
    maps_full = [torch.from_numpy(m.copy()).cuda() for m in want_maps]
    zb, ze = 5, 14  # odd begin, 9 planes: a short last plane block
    region = ((zb, ze), (0, want_lo.shape[2]), (0, want_lo.shape[3]))
    fill = 0xA5A5
    for rev, tail in itertools.product((0, 1), (0, 32, 512, 8192)):
        kmp_opt('KMP_W3_DEC_REV', rev)
        kmp_opt('KMP_W3_ST_TAIL', tail)
        lo = torch.full_like(lo_full, fill)
        maps = [torch.full_like(m, fill) for m in maps_full]
        _nd.fused_encode_into(xd, pred, coder, lo, maps, 3, region=region)
        assert _last(kom) == 'wave3d_encode'
        for got, full in zip((lo, *maps), (lo_full, *maps_full)):
            want = torch.full_like(full, fill)
            want[:, zb:ze] = full[:, zb:ze]
            assert torch.equal(got, want), (rev, tail)
        rec = torch.full_like(xd, fill)
        _nd.fused_decode_into(lo_full, maps_full, dims, pred, coder, rec, 3, region=region)
        assert _last(kom) == 'wave3d_decode'
        want = torch.full_like(xd, fill)
        want[:, 2 * zb:2 * ze] = xd[:, 2 * zb:2 * ze]
        assert torch.equal(rec, want), (rev, tail)


@pytest.mark.parametrize('setting', ['defaults', 'rev_tail'])
def test_plan_replay_matches_eager(kom, kmp_opt, setting):
    """CodecPlan graph replay of the C3 tile shape is bit-identical to eager, with the library's
    defaults and with the reversed decode and a cached tail of half the batch."""
    if setting == 'rev_tail':
        kmp_opt('KMP_W3_DEC_REV', 1)
        kmp_opt('KMP_W3_ST_TAIL', 2048)
    x, want_lo, want_maps, _ = _reference('tile64x8')
    pred = kom.MeanPredictor(0, 3)
    plan = kom.graphs.CodecPlan(pred, x.shape, torch.uint16)
    xd = torch.from_numpy(x.copy()).cuda()
    for rep in range(2):
        lo, (maps, dims) = plan.encode(xd)
        assert np.array_equal(lo.cpu().numpy(), want_lo)
        assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(maps, want_maps))
        assert torch.equal(plan.decode(), xd)
    e_lo, (e_maps, e_dims) = kom.volume.encode(pred, kom.volume.encode_values_uint16, xd)
    assert _last(kom) == 'wave3d_encode'
    assert torch.equal(e_lo, lo) and all(torch.equal(a, b) for a, b in zip(e_maps, maps))
    assert torch.equal(kom.volume.decode(pred, kom.volume.decode_values_uint16, e_lo, (e_maps, e_dims)), xd)
    assert _last(kom) == 'wave3d_decode'
