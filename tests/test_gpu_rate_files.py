"""Rate-controlled files: ``compress(target_bits=...)`` against tests/rate_spec.py.

The ground truth for sizes is the explicit-bound path (``compress(abs_error=...)`` / ``rel_error`` /
``max_error``): a rung's file written with its bound, and ``rate_spec.bound_bytes_of`` of it.  The rung
a target chooses must be the one ``rate_spec.search`` chooses on those sizes, every probe the product
reports must equal the ground truth of its rung, and the file must be that rung's file, byte for byte.
Ground-truth files are written on demand -- only for the rungs the search asks -- and kept per case."""

import filecmp
import json
import os

import numpy as np
import pytest
import torch

import near_spec as NS
import quant_spec as Q
import rate_spec as R
import signed_spec as SS

pytestmark = pytest.mark.gpu

VOL, IMG = (1, 20, 24, 33, 1), (2, 21, 18, 1)
LEVELS = 2


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def field(shape, variant, seed=0):
    """test_gpu_quant_files.field: smooth -- a smooth float32 field under a little noise; exceptions -- with
    a NaN block, both infinities, NaN payloads and one value past the int32 range."""
    rng = np.random.default_rng(seed)
    x = np.empty(shape, np.float64)
    for b in range(shape[0]):
        x[b, ..., 0] = 3.0 * SS.smooth_field(shape[1:-1], seed + b) + 0.01 * rng.standard_normal(shape[1:-1])
    x = x.astype(np.float32)
    if variant == 'exceptions':
        ndim = len(shape) - 2
        x[(0, *[slice(s // 3, s // 3 + 3) for s in shape[1:1 + ndim]])] = np.nan
        f = x.reshape(-1)
        f[[0, 7, f.size - 1]] = [np.inf, -np.inf, 3e38]
        u32(f)[[f.size // 2, f.size // 2 + 1]] = [0x7fc00001, 0xffc12345]
    return x


# (id, mode, the data, the two neighbouring rungs (indices into the ladder) the budgets are taken from)
def _cases():
    fv, fi = field(VOL, 'smooth'), field(IMG, 'smooth', seed=3)
    return {
        'abs-vol': ('abs', fv, R.ladder_abs(R.largest_finite(fv)), 16),
        'rel-img': ('rel', fi, R.ladder_rel(), 11),
        'near-u16-vol': ('near', NS.noisy_field(VOL, np.uint16, seed=1), R.ladder_near(np.uint16), 2),
        'near-u8-img': ('near', NS.noisy_field(IMG, np.uint8, seed=2), R.ladder_near(np.uint8), 1),
    }


CASE_IDS = ['abs-vol', 'rel-img', 'near-u16-vol', 'near-u8-img']


class Truth:
    """The explicit-bound files of one case, written when first asked for."""

    def __init__(self, kom, root, name, tile_crc):
        self.kom, self.name, self.tile_crc = kom, name, tile_crc
        self.mode, self.x, self.ladder, self.at = _cases()[name]
        self.P = kom.MeanPredictor(0, self.x.ndim - 2)
        self.dir = root / name
        self.dir.mkdir()
        self.sizes, self.infos = {}, {}

    def path(self, r):
        return str(self.dir / f'rung{r}.kmp')

    def size(self, r):
        if r not in self.sizes:
            self.infos[r] = self.kom.container.compress(self.path(r), self.x, self.P, levels=LEVELS, tile_crc=self.tile_crc,
                                                        **R.bound_kw(self.mode, self.ladder[r]))
            self.sizes[r] = R.bound_bytes_of(self.path(r))
            assert os.path.getsize(self.path(r)) <= self.sizes[r] <= os.path.getsize(self.path(r)) + 16
        return self.sizes[r]

    def target(self, path, budget, **kw):
        """compress under a budget of exactly ``budget`` bytes (the half byte keeps the floor off the edge)."""
        bits = 8.0 * (budget + 0.5) / self.x.size
        out = self.kom.container.compress(path, self.x, self.P, levels=LEVELS, tile_crc=self.tile_crc,
                                          target_bits=bits, **({'target_mode': self.mode} if self.mode == 'rel' else {}), **kw)
        assert out['target_bytes'] == budget == R.budget(self.x.size, self.x.nbytes, target_bits=bits)
        return out

    def within_bound(self, restored, value):
        x, r = self.x.astype(np.float64), np.asarray(restored).astype(np.float64)
        assert restored.dtype == self.x.dtype and restored.shape == self.x.shape
        if self.mode == 'abs':
            assert np.abs(r - x).max() <= 2.0 ** (value - 1)
        elif self.mode == 'rel':
            assert (np.abs(r - x) <= 2.0 ** -(value + 1) * np.maximum(np.abs(x), 2.0 ** -126)).all()
        else:
            assert np.abs(r - x).max() <= value


@pytest.fixture(scope='module')
def truths(kom, tmp_path_factory):
    root = tmp_path_factory.mktemp('rate_truth')
    return {name: Truth(kom, root, name, tile_crc=(i % 2 == 0)) for i, name in enumerate(CASE_IDS)}


@pytest.mark.parametrize('name', CASE_IDS)
def test_a_target_picks_the_specs_rung_and_writes_its_file(kom, truths, tmp_path, name):
    t = truths[name]
    L, a = len(t.ladder), t.at
    sa, sb = t.size(a), t.size(a + 1)
    print(f'{name}: rungs {t.ladder[a]} / {t.ladder[a + 1]}: {sa} / {sb} bytes')
    assert sa != sb, 'the two rungs the budgets come from must differ in size'
    for budget in (sb, sb - 1, (sa + sb) // 2):
        want, probes = R.search(t.size, L, budget)
        path = str(tmp_path / f'b{budget}.kmp')
        out = t.target(path, budget)
        print(f'  budget {budget}: rung {t.ladder[want]}, {len(probes)} probes, file {os.path.getsize(path)} bytes')
        assert out['probes'] == [(t.ladder[r], s) for r, s in probes]
        assert len(out['probes']) <= R.max_probes(L)
        assert out['bound_bytes'] == t.size(want) <= budget
        assert want == 0 or t.size(want - 1) > budget
        assert filecmp.cmp(path, t.path(want), shallow=False), 'not the explicit-bound file of the chosen rung'
        assert os.path.getsize(path) == out['bytes'] <= budget
        explicit = t.infos[want]
        assert {k: out[k] for k in explicit} == explicit  # the explicit call's result, plus the three keys
        assert set(out) - set(explicit) == {'target_bytes', 'bound_bytes', 'probes'}
        assert not [f for f in os.listdir(tmp_path) if '.tmp' in f]
        t.within_bound(kom.container.decompress(path), t.ladder[want])


@pytest.mark.parametrize('name', CASE_IDS)
def test_the_ends_of_the_ladder(kom, truths, tmp_path, name):
    t = truths[name]
    L = len(t.ladder)
    coarsest = t.size(L - 1)
    path = str(tmp_path / 'never.kmp')
    with pytest.raises(ValueError) as e:
        t.target(path, coarsest - 1)
    assert str(coarsest) in str(e.value)
    assert os.listdir(tmp_path) == []  # neither the file nor a temporary
    out = t.target(path, coarsest)  # exactly the coarsest rung's size is reachable
    assert out['bound_bytes'] <= coarsest and os.path.getsize(path) <= coarsest
    finest = t.size(0)
    out = t.target(path, finest + 5, **({} if t.mode == 'rel' else {'target_mode': t.mode}))  # the default mode, named
    assert out['probes'] == [(t.ladder[0], finest)] and out['bound_bytes'] == finest
    assert filecmp.cmp(path, t.path(0), shallow=False)
    if t.mode == 'near':
        assert out['max_error'] == 0 and np.array_equal(kom.container.decompress(path), t.x)  # rung 0 is lossless


def test_target_ratio_is_the_same_budget(kom, truths, tmp_path):
    t = truths['abs-vol']
    sb = t.size(t.at + 1)
    ratio = t.x.nbytes / (sb + 0.5)
    assert R.budget(t.x.size, t.x.nbytes, target_ratio=ratio) == sb
    out = kom.container.compress(str(tmp_path / 'r.kmp'), t.x, t.P, levels=LEVELS, tile_crc=t.tile_crc, target_ratio=ratio)
    want, probes = R.search(t.size, len(t.ladder), sb)
    assert out['target_bytes'] == sb and out['probes'] == [(t.ladder[r], s) for r, s in probes]
    assert filecmp.cmp(str(tmp_path / 'r.kmp'), t.path(want), shallow=False)
    assert out['ratio'] >= ratio


SIZED = [('lossless-u16', NS.noisy_field, np.uint16, {}), ('lossless-f32', None, np.float32, {}),
         ('near', NS.noisy_field, np.uint16, {'max_error': 3}), ('near-i8', NS.noisy_field, np.int8, {'max_error': 2}),
         ('abs', None, np.float32, {'abs_error': 1e-3}), ('rel', None, np.float32, {'rel_error': 1e-3})]


@pytest.mark.parametrize('tile_crc', [False, True], ids=['plain', 'tile_crc'])
@pytest.mark.parametrize('shape', [VOL, IMG], ids=['vol', 'img'])
@pytest.mark.parametrize('case', SIZED, ids=[c[0] for c in SIZED])
def test_compressed_size_is_the_files(kom, tmp_path, case, shape, tile_crc):
    _, make, dtype, bound = case
    x = field(shape, 'exceptions') if make is None else make(shape, dtype, seed=4)
    P = kom.MeanPredictor(0, len(shape) - 2)
    path = str(tmp_path / 'f.kmp')
    info = kom.container.compress(path, x, P, levels=LEVELS, tile_crc=tile_crc, **bound)
    before = sorted(os.listdir(tmp_path))
    got = kom.container.compressed_size(x, P, levels=LEVELS, tile_crc=tile_crc, **bound)
    assert sorted(os.listdir(tmp_path)) == before  # it writes nothing
    with open(path, 'rb') as f:
        head = f.read(16)
        meta = json.loads(f.read(int.from_bytes(head[8:16], 'little')))
    print(f'{case[0]} {shape} tile_crc={tile_crc}: file {info["bytes"]}, sized {got}')
    assert got['bound_bytes'] == R.bound_bytes_of(path)
    assert info['bytes'] <= got['bound_bytes'] <= info['bytes'] + 16
    assert got['bundle_bytes'] == meta['bundle_bytes']
    assert got['raw_bytes'] == info['raw_bytes'] == x.nbytes and got['levels'] == info['levels'] == LEVELS
    for key in ('max_error', 'abs_error', 'rel_error', 'exceptions', 'quant_dtype'):
        assert (key in got) == (key in info) and got.get(key) == info.get(key), key
    if dtype == np.float32 and bound:
        assert got['exceptions'] > 0
    again = kom.container.compressed_size(torch.from_numpy(x).cuda(), P, levels=LEVELS, tile_crc=tile_crc, **bound)
    assert again == got  # a device input, and measured twice


_SPEC = {}


def spec_field():
    if 'x' not in _SPEC:
        _SPEC['x'] = Q.spec_field()
    return _SPEC['x']


@pytest.mark.parametrize('bits', [4, 6, 9])
def test_target_bits_on_the_spec_field(kom, tmp_path, bits):
    """The oracle puts this field's ladder at 0.25 - 13.4 bits per sample (MeanPredictor(0), 2 levels), so
    4, 6 and 9 bits lie inside it: each succeeds and the file is no larger than asked."""
    x = spec_field()
    assert x.shape == (1, 40, 48, 56, 1)
    path = str(tmp_path / 's.kmp')
    out = kom.container.compress(path, x, kom.MeanPredictor(0, 3), levels=2, target_bits=bits)
    print(f'target {bits} bits: {out["bits_per_sample"]:.3f} bits, abs_error {out["abs_error"]}, probes {out["probes"]}')
    assert out['bits_per_sample'] <= bits and 8.0 * os.path.getsize(path) / x.size <= bits
    assert out['target_bytes'] == bits * x.size // 8 and len(out['probes']) <= R.max_probes(32)
    r = kom.container.decompress(path)
    assert np.abs(r.astype(np.float64) - x.astype(np.float64)).max() <= out['abs_error']
    finer = kom.container.compressed_size(x, kom.MeanPredictor(0, 3), levels=2, abs_error=out['abs_error'] / 2)
    assert finer['bound_bytes'] > out['target_bytes']  # the next finer rung does not fit
