"""The Rice path model against the specification, and the census of the paths its generated
bundles reach (CPU only).  The GPU suite (``test_gpu_rice_paths.py``) runs exactly these bundles:
what is asserted here is what it covers."""

from collections import Counter

import numpy as np
import pytest

from oracle import rice as R
import rice_spec as S

MIN_PER_BUCKET = 8


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.fixture(scope='module')
def corpus():
    return {W: ([S.reach_bundle(W, i) for i in range(S.NBUNDLES)],
                [S.forced_bundle(W, i) for i in range(S.NBUNDLES)]) for W in S.WS}


@pytest.mark.parametrize('W', S.WS)
def test_unforced_packer_is_the_specification(corpus, W):
    """With every k left to k*, ``pack_forced`` and ``pack_bundle_forced`` return the oracle's bytes."""
    reach, forced = corpus[W]
    for arrays in reach + [a for a, _ in forced]:
        for a in arrays:
            for got, want in zip(S.pack_forced(a), R.pack(a)):
                assert got.dtype == want.dtype and np.array_equal(got, want)
            assert all(np.array_equal(g, w) for g, w in zip(S.pack_forced(a, [None] * (-(-a.size // 64))), R.pack(a)))
        assert np.array_equal(S.pack_bundle_forced(arrays, [None] * len(arrays), (4, 6)), R.pack_bundle(arrays, (4, 6)))


@pytest.mark.parametrize('W', S.WS)
def test_forced_bundles_decode_to_their_source(corpus, W):
    """Every forced bundle is a valid bundle of its arrays: the specification's decoder returns them,
    the side information lies within the format's bounds, and the bytes differ from the encoder's."""
    for arrays, ks in corpus[W][1]:
        blob = S.pack_bundle_forced(arrays, ks)
        back, dims = R.unpack_bundle(blob)
        assert dims == () and len(back) == len(arrays)
        assert all(_same(b, a) for a, b in zip(arrays, back))
        assert not np.array_equal(blob, R.pack_bundle(arrays))
        for a, k in zip(arrays, ks):
            params, bw, _ = S.pack_forced(a, k)
            kk = params.astype(np.int64) - 1
            coded = params > 0
            assert (bw[~coded] == 0).all() and (kk[coded] < W).all()
            assert (bw[coded] >= 2 * kk[coded] + 2).all() and (bw[coded] <= 2 * W + 2).all()


def test_forced_packer_rejects_what_the_format_does():
    x = np.arange(64, dtype=np.uint8)
    with pytest.raises(AssertionError):
        S.pack_forced(x, [-1])        # param 0 on a block that is not all zero
    with pytest.raises(AssertionError):
        S.pack_forced(x, [0])         # k = 0 needs more than 2W + 2 words
    with pytest.raises(AssertionError):
        S.pack_forced(x, [8])         # k >= W


@pytest.mark.parametrize('W', S.WS)
def test_encoder_never_writes_a_long_stream(corpus, W):
    """The lemma at ``short_stream`` in kmp_rice.hip: uw(k*) <= 7 (<= 4 at k* = W - 1) on every
    generated block, the forced bundles' blocks taken at their k* as well -- so the decoders'
    ``!short_stream`` walk and a terminator in stream word 7 are reached by forced parameters only."""
    reach, forced = corpus[W]
    seen = 0
    for arrays in reach + [a for a, _ in forced]:
        for a in arrays:
            f = S.classify(a)
            for k, uw in zip(f['k'][f['coded']], f['uw'][f['coded']]):
                assert uw <= S.unary_words_bound(W, int(k)), (W, int(k), int(uw))
            seen = max(seen, int(f['uw'].max()))
    assert seen == 7  # the bound is met


@pytest.mark.parametrize('W', S.WS)
def test_census(corpus, W):
    """Every required bucket holds at least 8 elements (blocks, lanes, samples or steps, as the
    bucket says) over the 8 bundles of this width: those of encoder-reachable data in the bundles the
    kernels pack, those of forced parameters in the forced bundles."""
    reach, forced = corpus[W]
    cr, cf = Counter(), Counter()
    for arrays in reach:
        for a in arrays:
            cr += S.census(a)
    for arrays, ks in forced:
        for a, k in zip(arrays, ks):
            cf += S.census(a, k)
    print(f'\nW={W} encoder-reachable: {S.format_census(cr, S.required_reach(W))}')
    print(f'W={W} forced: {S.format_census(cf, S.required_forced(W))}')
    short = {b: cr.get(b, 0) for b in S.required_reach(W) if cr.get(b, 0) < MIN_PER_BUCKET}
    short.update({b: cf.get(b, 0) for b in S.required_forced(W) if cf.get(b, 0) < MIN_PER_BUCKET})
    assert not short, (W, short)
    # the encoder's data takes no long path at all
    assert cr['dec long step'] == 0 and cr['uw=8, terminator 8j-1 in word 7'] == 0


def _ends_on(n, i):
    """n ends on size kind i: a multiple of 8 / 64 / 512 / 16384 and of no coarser unit, plus i % 2."""
    base = n - i % 2
    unit = (8, 64, 512, S.TILE_SAMPLES)[i // 2]
    finer = (64, 512, S.TILE_SAMPLES, None)[i // 2]
    return base % unit == 0 and (finer is None or base % finer != 0)


@pytest.mark.parametrize('W', S.WS)
def test_bundle_sizes(corpus, W):
    """Bundle i's main array, encoder-reachable and forced, ends on size kind i: a lane, a block, a
    wave step and a tile boundary and one sample past each; every small array ends inside a lane of
    a step whose tail lies past nb."""
    reach, forced = corpus[W]
    for i in range(S.NBUNDLES):
        (arrays, ks), mains = forced[i], (reach[i][0], forced[i][0][0])
        assert all(_ends_on(a.size, i) for a in mains), (i, [a.size for a in mains])
        for small in (reach[i][1], arrays[1]):
            assert small.size % 8 and -(-small.size // 64) % 8
        assert len(ks[0]) == -(-arrays[0].size // 64) and ks[1] is None


def test_sparse_tiles():
    """The look-back bundles: every tile holds coded blocks, neighbouring tiles differ in word count."""
    x = S.sparse_tiles(9, np.uint16, 0)
    params, bw, _ = R.pack(x)
    per = bw.astype(np.int64).reshape(9, -1).sum(axis=1)
    assert (per > 0).all() and (np.diff(per) != 0).all()
