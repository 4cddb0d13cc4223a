"""Guard bands, exact ownership and off-alignment pointers for the packers, the Rice bundle coder,
the moment accumulation of the fit and the CRC (kmp_pack.hip, kmp_rice.hip, kmp_fit.hip, kmp_crc.hip),
called through ``kompressor_amd._lib.lib`` with every tensor -- samples, widths, workspace at exactly
its ``*_workspace_bytes``, the payload sized by the plan, the outputs at exactly n samples -- in a
sentinel-filled arena of its own (guard_capi.py).  Checks as in test_gpu_guard_primitives.py; where
the header states an alignment (payload and workspaces 8 bytes, crc data 16) the pointer moves by that
instead of by one element.  Expected bytes: oracle.packing, oracle.rice, fit_spec, zlib."""

import struct
import zlib

import numpy as np
import pytest

from oracle import packing as OPK
from oracle import rice as OR
import fit_spec
import guard_capi as K
from guard_capi import T, CODE

pytestmark = pytest.mark.gpu

LAUNCHES = ('kmp_pack_plan', 'kmp_pack', 'kmp_pack_header', 'kmp_unpack_plan', 'kmp_unpack', 'kmp_unpack_check',
            'kmp_rice_bundle_encode', 'kmp_rice_bundle_decode', 'kmp_linear_moments', 'kmp_crc32')

INTS = [np.uint8, np.uint16, np.int32]
INT_IDS = ['uint8', 'uint16', 'int32']


def residuals(n, dtype, seed):
    """Coder-like samples: small signed residuals (modular for the unsigned dtypes), one block of 64
    full-range values, one all-zero block -- every block width, a zero block, a ragged last block."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-40, 41, size=n).astype(np.int64)
    if n > 128:
        x[64:128] = K.rand((64,), dtype, seed + 1).astype(np.int64)
    if n > 256:
        x[192:256] = 0
    if n == 1:
        x[0] = -3
    return x.astype(dtype)  # negative values wrap into the unsigned dtypes


def _lib():
    from kompressor_amd import _lib
    return _lib.lib


# ---------------------------------------------------------------------------------------------
# bit-plane packer: plan -> pack -> unpack_plan -> unpack (-> check, header)
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n', [1, 63, 64, 65, 1000])
@pytest.mark.parametrize('dtype', INTS, ids=INT_IDS)
def test_pack_chain(kom, dtype, n):
    lib = _lib()
    code = CODE[np.dtype(dtype)]
    x = residuals(n, dtype, n)
    widths, payload = OPK.pack(x)
    assert np.array_equal(OPK.unpack(widths, payload, n, dtype), x)
    nb, words = len(widths), int(widths.astype(np.int64).sum())
    assert nb == lib.kmp_pack_blocks(n) and payload.size == words and words > 0
    ws_bytes, total_off = int(lib.kmp_pack_workspace_bytes(n)), int(lib.kmp_pack_total_offset(n))
    ws_shape = np.zeros(ws_bytes, np.uint8)
    payload_bytes = payload.view(np.uint8)

    for shift in K.SHIFTS:
        # the plan: widths of x, the block offsets and the payload's word count into the workspace
        keep = []
        name = K.launch('kmp_pack_plan', [T('x', 'in', x), T('widths', 'out', widths),
                                          T('workspace', 'scratch', ws_shape, align=8)],
                        lambda fn, p: fn(code, p['x'], n, p['widths'], p['workspace'], None), shift, keep=keep)
        assert name == 'pack_scan'
        plans = [K.payload_numpy(got['workspace']) for got in keep]
        for ws in plans:
            assert struct.unpack('<Q', ws[total_off:total_off + 8].tobytes())[0] == words
        # the payload, sized by the plan, from the workspace that plan launch left
        name = K.launch('kmp_pack', [T('x', 'in', x), T('widths', 'in', widths),
                                     T('workspace', 'in', plans[0], align=8),
                                     T('payload', 'out', payload_bytes, align=8)],
                        lambda fn, p: fn(code, p['x'], n, p['widths'], p['workspace'], p['payload'], None), shift)
        assert name == 'pack'
        # the decoder's plan from the stored widths alone
        keep = []
        name = K.launch('kmp_unpack_plan', [T('widths', 'in', widths), T('workspace', 'scratch', ws_shape, align=8)],
                        lambda fn, p: fn(p['widths'], n, p['workspace'], None), shift, keep=keep)
        assert name == 'pack_scan'
        uplans = [K.payload_numpy(got['workspace']) for got in keep]
        for ws in uplans:
            assert struct.unpack('<Q', ws[total_off:total_off + 8].tobytes())[0] == words
        name = K.launch('kmp_unpack', [T('payload', 'in', payload_bytes, align=8), T('widths', 'in', widths),
                                       T('workspace', 'in', uplans[0], align=8), T('out', 'out', x)],
                        lambda fn, p: fn(code, p['payload'], n, p['widths'], p['workspace'], p['out'], None), shift)
        assert name == 'unpack'


@pytest.mark.parametrize('n', [1, 63, 64, 65, 1000])
def test_unpack_check_and_header(kom, n):
    """kmp_unpack_check owns the 8 bytes after the plan's total in the workspace (the count of blocks
    whose side information no encoder writes); kmp_pack_header owns dst[0, len), the zero range and the
    8 bytes at ``words_at``."""
    lib = _lib()
    rng = np.random.default_rng(n)
    nb = int(lib.kmp_pack_blocks(n))
    ws_bytes, total_off = int(lib.kmp_pack_workspace_bytes(n)), int(lib.kmp_pack_total_offset(n))
    own = np.zeros(ws_bytes, bool)
    own[total_off + 8:total_off + 16] = True
    for fmt, W, code in ((0, 8, 0), (0, 16, 1), (1, 16, 1), (1, 32, 2)):
        if fmt == 0:
            a = rng.integers(0, W + 3, size=nb).astype(np.uint8)  # widths, some past W
            b = np.zeros(nb, np.uint8)
            bad = int((a > W).sum())
        else:
            a = rng.integers(0, W + 2, size=nb).astype(np.uint8)  # k + 1, some with k >= W
            b = rng.integers(0, 2 * W + 5, size=nb).astype(np.uint8)
            k, wd = a.astype(np.int64) - 1, b.astype(np.int64)
            bad = int(np.where(a == 0, wd != 0, (k >= W) | (wd < 2 * k + 2) | (wd > 2 * W + 2)).sum())
        want = np.zeros(ws_bytes, np.uint8)
        want[total_off + 8:total_off + 16] = np.frombuffer(struct.pack('<Q', bad), np.uint8)
        for shift in K.SHIFTS + ({'side_a': 8, 'side_b': 8, 'workspace': 8},):  # the 8-byte loads' turn
            name = K.launch('kmp_unpack_check', [T('side_a', 'in', a), T('side_b', 'in', b),
                                                 T('workspace', 'out', want, mask=own, align=8)],
                            lambda fn, p: fn(fmt, code, p['side_a'], p['side_b'] if fmt else None, n, p['workspace'],
                                             None), shift)
            assert name == 'unpack_check'
    # the header: bytes from the host, a zero range, the plan's word count from the workspace
    head = bytes(rng.integers(0, 256, size=37).astype(np.uint8))
    ws = rng.integers(0, 256, size=ws_bytes).astype(np.uint8)
    words = 0x0123456789ABCDEF
    ws[total_off:total_off + 8] = np.frombuffer(struct.pack('<Q', words), np.uint8)
    for zf, zt, at in ((40, 61, 64), (37, 37, -1), (100, 131, 37)):
        want, own = np.zeros(160, np.uint8), np.zeros(160, bool)
        want[:37], own[:37] = np.frombuffer(head, np.uint8), True
        own[zf:zt] = True
        if at >= 0:
            want[at:at + 8], own[at:at + 8] = np.frombuffer(struct.pack('<Q', words), np.uint8), True
        for shift in K.SHIFTS:
            name = K.launch('kmp_pack_header', [T('workspace', 'in', ws, align=8), T('dst', 'out', want, mask=own)],
                            lambda fn, p: fn(p['dst'], head, len(head), zf, zt, p['workspace'] if at >= 0 else None, n,
                                             at, None), shift)
            assert name == 'pack_header'


# ---------------------------------------------------------------------------------------------
# Rice bundle
# ---------------------------------------------------------------------------------------------

BUNDLE_NS = (65, 16384 + 1, 1)  # the middle array crosses the 256-block tile boundary


def _bundle_arrays(dtype, ns=BUNDLE_NS):
    return [residuals(n, dtype, 17 * i + n) for i, n in enumerate(ns)]


@pytest.mark.parametrize('dtype', INTS, ids=INT_IDS)
def test_rice_bundle_encode(kom, dtype):
    """One launch of three arrays, laid out as the product lays it out (packing._rice_enc_plan,
    packing._rice_arrays_n) in a bundle arena of the product's capacity, payload_off + worst + 8 with
    worst = sum over the arrays of ceil(n / 64) * (2 W + 2) * 4 bytes.  Bytes [0, total) are the
    oracle's bundle, in both runs; total <= payload_off + worst; and the launch writes no byte at or
    past ``total`` (the capacity contract the header states): the highest byte it changes is below it."""
    import torch
    from kompressor_amd import packing
    arrays = _bundle_arrays(dtype)
    blob = OR.pack_bundle(arrays)
    total = blob.size
    plan = packing._rice_enc_plan([torch.from_numpy(a.view(np.uint8)).cuda().view(K.NP2T[np.dtype(dtype)])
                                   for a in arrays], ())
    poff, head, capacity = plan['poff'], plan['head'], plan['poff'] + plan['worst'] + 8
    assert (head, plan['offs'], poff) == OR.bundle_layout(list(BUNDLE_NS)) and plan['T'] == 4
    assert struct.unpack('<Q', blob[64:72].tobytes())[0] == total <= poff + plan['worst']
    hdr = plan['hdr'].cpu().numpy()
    assert hdr.size == head
    names = [f'x{i}' for i in range(len(arrays))]
    for shift in K.SHIFTS:
        keep = []

        def prepare(got):  # the header is the caller's part of the bundle
            c = got['bundle']
            c.arena[K.G.GUARD + c.shift:K.G.GUARD + c.shift + head].copy_(torch.from_numpy(hdr))

        def call(fn, p):
            arr = packing._rice_arrays_n(plan['ns'], plan['offs'], 0, len(arrays), [p[nm] for nm in names])
            return fn(CODE[np.dtype(dtype)], arr, len(arrays), 0, plan['T'], p['bundle'], poff, p['workspace'], None)

        # the bundle is prepared by the caller and written by the launch: the harness checks its guards
        # (role 'scratch'), the lines below its bytes
        name = K.launch('kmp_rice_bundle_encode',
                        [T(nm, 'in', a) for nm, a in zip(names, arrays)]
                        + [T('bundle', 'scratch', np.zeros(capacity, np.uint8), align=8),
                           T('workspace', 'scratch', np.zeros(plan['ws_bytes'], np.uint8), align=8)],
                        call, shift, keep=keep, prepare=prepare)
        assert name == 'rice_bundle_encode'
        runs = [K.payload_numpy(got['bundle']) for got in keep]
        for got in runs:
            assert np.array_equal(got[:total], blob)
        changed = np.zeros(capacity, bool)
        for got, c in zip(runs, keep):
            changed |= got != c['bundle'].sentinel  # a byte written with one run's sentinel shows in the other
        top = int(np.flatnonzero(changed).max())
        print(f'rice_bundle_encode {np.dtype(dtype).name} shift {shift}: highest byte written {top}, total {total}, '
              f'capacity {capacity}')
        assert top < total, f'highest byte written {top}, total {total}, capacity {capacity}'


@pytest.mark.parametrize('ns', [BUNDLE_NS, (63,), (64,), (16383,), (16384,)], ids=lambda v: 'x'.join(map(str, v)))
@pytest.mark.parametrize('dtype', INTS, ids=INT_IDS)
def test_rice_bundle_decode(kom, dtype, ns):
    """The oracle's bundle (an input, at exactly its size: unchanged) decoded into output arenas of
    exactly n samples each -- n = 65 and n = 1 are where a 4-byte store of 1 / 2-byte samples overruns;
    the bad-tile counter stays 0."""
    from kompressor_amd import packing
    arrays = _bundle_arrays(dtype, ns)
    blob = OR.pack_bundle(arrays)
    back, _ = OR.unpack_bundle(blob)
    assert all(np.array_equal(a, b) for a, b in zip(arrays, back))
    _, offs, poff = OR.bundle_layout(list(ns))
    words = struct.unpack('<Q', blob[56:64].tobytes())[0]
    names = [f'x{i}' for i in range(len(arrays))]
    for shift in K.SHIFTS:
        def call(fn, p):
            arr = packing._rice_arrays_n(list(ns), offs, 0, len(ns), [p[nm] for nm in names])
            return fn(CODE[np.dtype(dtype)], arr, len(ns), 0, p['bundle'], poff, words, p['bad'], None)

        name = K.launch('kmp_rice_bundle_decode',
                        [T('bundle', 'in', blob, align=8), T('bad', 'in', np.zeros(1, np.int64))]
                        + [T(nm, 'out', a) for nm, a in zip(names, arrays)], call, shift)
        assert name == 'rice_bundle_decode'


# ---------------------------------------------------------------------------------------------
# the fit's moments, the CRC
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize('nsp,shape,dtype,p', [(3, (2, 5, 6, 9, 1), np.uint8, 0), (3, (2, 5, 6, 9, 1), np.uint8, 1),
                                               (3, (2, 5, 6, 9, 1), np.uint16, 0), (3, (2, 5, 6, 9, 1), np.uint16, 1),
                                               (2, (3, 9, 10, 1), np.uint8, 2), (2, (3, 9, 10, 1), np.uint16, 2)])
def test_linear_moments(kom, nsp, shape, dtype, p):
    lib = _lib()
    h = K.rand(shape, dtype, 31 + p)
    M = fit_spec.spec_moments(h, p, nsp)
    need = int(lib.kmp_linear_moments_workspace_bytes(nsp, CODE[np.dtype(dtype)], p))
    assert need > 0 and M.dtype == np.int64
    for shift in K.SHIFTS:
        name = K.launch('kmp_linear_moments', [T('highres', 'in', h), T('moments', 'out', M, align=8),
                                               T('workspace', 'scratch', np.zeros(need, np.uint8), align=8)],
                        lambda fn, q: fn(nsp, CODE[np.dtype(dtype)], q['highres'], shape[0], K.i64x3(shape[1:1 + nsp]),
                                         1, p, q['moments'], q['workspace'], None), shift)
        assert name.startswith('linear_moments')


@pytest.mark.parametrize('n', [1, 15, 16, 17, 70000])
def test_crc32(kom, n):
    """The 4-byte result in an arena; the length from the host, and (n > 1) a shorter one read from a
    device int64."""
    data = K.rand((n,), np.uint8, n)
    for shift in K.SHIFTS:
        want = np.array([zlib.crc32(data.tobytes())], np.uint32)
        name = K.launch('kmp_crc32', [T('data', 'in', data, align=16), T('crc', 'out', want)],
                        lambda fn, p: fn(p['data'], n, None, p['crc'], None), shift)
        assert name == 'crc32'
        if n > 1:
            m = n - n // 3 - 1
            want = np.array([zlib.crc32(data[:m].tobytes())], np.uint32)
            K.launch('kmp_crc32', [T('data', 'in', data, align=16), T('n_dev', 'in', np.array([m], np.int64)),
                                   T('crc', 'out', want)],
                     lambda fn, p: fn(p['data'], n, p['n_dev'], p['crc'], None), shift)


def test_every_declared_entry_point_was_launched():
    """Runs last: the ledger counts LAUNCHES as guarded, so each of them must have run above."""
    K.assert_declared_were_launched(LAUNCHES)
