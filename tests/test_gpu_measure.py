"""The measuring mode of the Rice bundle encode (kmp_rice_bundle_encode with a NULL bundle) through
``packing.bundle_size`` / ``packing.encoded_size``: the size it reports is the length of the bundle the
real encode writes and of ``oracle.rice.pack_bundle``'s, for every sample width, at the sizes around
the block (64), the wave step (512) and the tile (16384), on all-zero, residual-like (the [-128, 127]
fast path), full-range (the general path, blocks of 2 W + 2 words) and mixed contents, on views at odd
element offsets and over several launches.  Signed arrays go to the oracle as their same-width unsigned
bits: the coder reads bits, and the oracle knows the unsigned codes only."""

import numpy as np
import pytest
import torch

from oracle import rice as OR

pytestmark = pytest.mark.gpu

DTYPES = [np.uint8, np.int8, np.uint16, np.int16, np.int32, np.uint32]
IDS = [np.dtype(d).name for d in DTYPES]
SIZES = [0, 1, 63, 64, 65, 16383, 16384, 16385, 2 * 16384 + 1]
CONTENTS = ['zero', 'residual', 'full', 'mixed']
BITS = {np.dtype(np.int8): np.uint8, np.dtype(np.int16): np.uint16}


def samples(n, dtype, content, seed=0):
    """zero: no payload; residual: every sample in [-128, 127] as a signed W-bit value (negative ones
    wrap in the unsigned dtypes); full: uniformly random bits; mixed: residuals with a full-range block,
    an all-zero block and a full-range stretch that ends inside a wave step."""
    rng = np.random.default_rng(seed + n)
    dtype = np.dtype(dtype)
    full = rng.integers(0, 2 ** (8 * dtype.itemsize), size=n, dtype=np.uint64)
    if content == 'zero':
        x = np.zeros(n, np.int64)
    elif content == 'residual':
        x = np.clip(np.rint(rng.laplace(0, 6, size=n)), -128, 127).astype(np.int64)
        if n:
            x[rng.integers(0, n, size=2)] = [-128, 127]
    elif content == 'full':
        x = full.astype(np.int64)
    else:
        x = np.clip(np.rint(rng.laplace(0, 3, size=n)), -128, 127).astype(np.int64)
        x[64:128] = full[64:128]
        x[192:256] = 0
        x[700:900] = full[700:900]        # ends inside the second wave step
        x[16384 - 100:16384 + 70] = full[16384 - 100:16384 + 70]  # across the tile boundary
        x[1024:1536:8] = 300               # one wave step of small values just past the byte range (W > 8)
    return x.astype(np.uint64).astype(f'u{dtype.itemsize}').view(dtype)  # modulo 2^W, then the dtype's reading


def oracle_size(arrays, dims=()):
    return int(OR.pack_bundle([a.view(BITS.get(a.dtype, a.dtype)) for a in arrays], dims).size)


def dev_of(a):
    return torch.from_numpy(a).cuda()


@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_size_is_the_bundles(kom, dtype, n):
    P = kom.packing
    for content in CONTENTS:
        x = samples(n, dtype, content)
        t = dev_of(x)
        want = oracle_size([x])
        real = P._rice_pack_bundle([t], ())
        got = P.bundle_size([t])
        print(f'{np.dtype(dtype).name} n={n} {content}: measured {got}, bundle {real.numel()}, oracle {want}')
        assert isinstance(got, int) and got == real.numel() == want, content
        assert P.bundle_size([x]) == got  # a numpy input
    if n == 0:
        assert P.bundle_size([dev_of(samples(0, dtype, 'zero'))]) == OR.bundle_layout([0])[2]  # payload_off alone


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_views_at_odd_element_offsets(kom, dtype):
    """The samples start 1 and 3 elements into an allocation: the 8- and 16-byte loads are unaligned."""
    n = 16384 + 65
    x = samples(n + 3, dtype, 'mixed', seed=5)
    t = dev_of(x)
    for off in (1, 3):
        v = t[off:off + n]
        assert v.is_contiguous() and v.data_ptr() == t.data_ptr() + off * x.dtype.itemsize
        want = oracle_size([x[off:off + n]])
        assert kom.packing.bundle_size([v]) == want == kom.packing._rice_pack_bundle([v], ()).numel()


def test_three_arrays_of_mixed_dtypes(kom):
    """Three runs, so three launches add into the one sum; the middle array spans three tiles."""
    arrays = [samples(1000, np.uint8, 'residual'), samples(2 * 16384 + 1, np.int32, 'mixed'),
              samples(16385, np.uint16, 'full')]
    ts = [dev_of(a) for a in arrays]
    assert len(kom.packing._rice_enc_plan(ts, (1, 0, 1))['runs']) == 3
    want = oracle_size(arrays, (1, 0, 1))
    assert kom.packing.bundle_size(ts, (1, 0, 1)) == want == kom.packing._rice_pack_bundle(ts, (1, 0, 1)).numel()


@pytest.mark.parametrize('count', [32, 33])
def test_32_arrays_are_one_launch_and_33_two(kom, count):
    ns = [(37 * i) % 700 + (16384 if i in (5, 32) else 0) for i in range(count)]  # n = 0 among them (i = 0)
    arrays = [samples(n, np.uint16, CONTENTS[i % 4], seed=i) for i, n in enumerate(ns)]
    ts = [dev_of(a) for a in arrays]
    assert len(kom.packing._rice_enc_plan(ts, ())['runs']) == (1 if count == 32 else 2)
    want = oracle_size(arrays)
    assert kom.packing.bundle_size(ts) == want == kom.packing._rice_pack_bundle(ts, ()).numel()


def test_two_measurements_agree_and_leave_the_encode_alone(kom):
    """Measured twice: the same number.  A real encode on the same stream before and after a
    measurement still writes the oracle's bytes."""
    arrays = [samples(16385, np.int32, 'mixed'), samples(70000, np.int32, 'residual'), samples(513, np.uint8, 'full')]
    ts = [dev_of(a) for a in arrays]
    want = OR.pack_bundle(arrays)
    P = kom.packing
    before = P._rice_pack_bundle(ts, ()).cpu().numpy()
    first = P.bundle_size(ts)
    after = P._rice_pack_bundle(ts, ()).cpu().numpy()
    second = P.bundle_size(ts)
    assert first == second == want.size
    assert np.array_equal(before, want) and np.array_equal(after, want)


def test_encoded_size(kom):
    rng = np.random.default_rng(2)
    vol = (np.cumsum(rng.integers(-3, 4, size=(2, 18, 20, 23, 1)), axis=3) + 1000).astype(np.uint16)
    pred = kom.MeanPredictor(0, 3)
    for data in (vol, torch.from_numpy(vol).cuda()):
        lo, enc = kom.volume.encode(pred, kom.volume.encode_values_uint16, data)
        blob = kom.packing.pack_encoded(lo, enc)
        assert kom.packing.encoded_size(lo, enc) == len(blob)
    for method in ('planes', 'huffman'):
        with pytest.raises(ValueError):
            kom.packing.encoded_size(lo, enc, method=method)
