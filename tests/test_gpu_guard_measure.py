"""Guard bands for the measuring mode of kmp_rice_bundle_encode (a NULL bundle, kmp_rice.hip
rice_bundle_measure_kernel), under the harness of guard_capi.py like test_gpu_guard_packing.py: the
samples are inputs at exactly n elements and come back unchanged at every pointer shift; the workspace,
at exactly ``kmp_rice_bundle_workspace_bytes``, is scratch between guards -- its first 8 bytes end as the
oracle's payload word count and no other byte of it changes; and ``kmp_last_launch`` tells the two modes
of the entry point apart."""

import struct

import numpy as np
import pytest

from oracle import rice as OR
import guard_capi as K
from guard_capi import T, CODE
from test_gpu_guard_packing import BUNDLE_NS, INTS, INT_IDS, _bundle_arrays

pytestmark = pytest.mark.gpu

LAUNCHES = ('kmp_rice_bundle_encode',)


def _plan(packing, arrays, dtype):
    import torch
    return packing._rice_enc_plan([torch.from_numpy(a.view(np.uint8)).cuda().view(K.NP2T[np.dtype(dtype)])
                                   for a in arrays], ())


@pytest.mark.parametrize('ns', [BUNDLE_NS, (63,), (16384,), (2 * 16384 + 1, 64)], ids=lambda v: 'x'.join(map(str, v)))
@pytest.mark.parametrize('dtype', INTS, ids=INT_IDS)
def test_rice_bundle_measure(kom, dtype, ns):
    from kompressor_amd import packing
    arrays = _bundle_arrays(dtype, ns)
    blob = OR.pack_bundle(arrays)
    words = struct.unpack('<Q', blob[56:64].tobytes())[0]
    assert words > 0
    plan = _plan(packing, arrays, dtype)
    ws_bytes = plan['ws_bytes']
    assert ws_bytes == kom._lib.lib.kmp_rice_bundle_workspace_bytes(plan['T']) >= 16
    names = [f'x{i}' for i in range(len(arrays))]
    for shift in K.SHIFTS:
        keep = []

        def call(fn, p):
            # layout offsets the mode ignores: deliberately not those of a bundle
            arr = packing._rice_arrays_n(plan['ns'], [(-8, 4)] * len(arrays), 0, len(arrays), [p[nm] for nm in names])
            return fn(CODE[np.dtype(dtype)], arr, len(arrays), 0, plan['T'], None, 12345, p['workspace'], None)

        name = K.launch('kmp_rice_bundle_encode',
                        [T(nm, 'in', a) for nm, a in zip(names, arrays)]
                        + [T('workspace', 'scratch', np.zeros(ws_bytes, np.uint8), align=8)],
                        call, shift, keep=keep)
        assert name == 'rice_bundle_measure'
        for got in keep:
            ws = K.payload_numpy(got['workspace'])
            assert struct.unpack('<Q', ws[:8].tobytes())[0] == words
            rest = ws[8:]
            assert (rest == got['workspace'].sentinel).all(), 'the launch wrote past the first 8 bytes of the workspace'


def test_a_real_encode_still_names_the_encode_kernel(kom):
    """The same entry point with a bundle: kmp_last_launch says rice_bundle_encode, and the bytes are the
    oracle's (test_gpu_guard_packing.py checks them under every shift; here the name, once)."""
    import torch
    from kompressor_amd import packing
    dtype = np.uint16
    arrays = _bundle_arrays(dtype)
    blob = OR.pack_bundle(arrays)
    plan = _plan(packing, arrays, dtype)
    poff, head, capacity = plan['poff'], plan['head'], plan['poff'] + plan['worst'] + 8
    hdr = plan['hdr'].cpu().numpy()
    names = [f'x{i}' for i in range(len(arrays))]
    keep = []

    def prepare(got):
        c = got['bundle']
        c.arena[K.G.GUARD + c.shift:K.G.GUARD + c.shift + head].copy_(torch.from_numpy(hdr))

    def call(fn, p):
        arr = packing._rice_arrays_n(plan['ns'], plan['offs'], 0, len(arrays), [p[nm] for nm in names])
        return fn(CODE[np.dtype(dtype)], arr, len(arrays), 0, plan['T'], p['bundle'], poff, p['workspace'], None)

    name = K.launch('kmp_rice_bundle_encode',
                    [T(nm, 'in', a) for nm, a in zip(names, arrays)]
                    + [T('bundle', 'scratch', np.zeros(capacity, np.uint8), align=8),
                       T('workspace', 'scratch', np.zeros(plan['ws_bytes'], np.uint8), align=8)],
                    call, 'none', keep=keep, prepare=prepare)
    assert name == 'rice_bundle_encode'
    for got in keep:
        assert np.array_equal(K.payload_numpy(got['bundle'])[:blob.size], blob)


def test_every_declared_entry_point_was_launched():
    """Runs last: each entry point this module declares must have run above."""
    K.assert_declared_were_launched(LAUNCHES)
