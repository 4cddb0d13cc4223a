"""The guard-band ledger: every function the C-ABI exports (``_lib.EXPORTED``, include/kompressor_hip.h)
that writes device memory is either launched under the guard harness -- by test_gpu_guard.py (the fused
calls) or by one of the test_gpu_guard_* modules, which declare their entry points in ``LAUNCHES`` and
each end with a test that every declared one really ran -- or stands on the short exemption list
below with its reason.  An entry point added to the C-ABI fails here until it gets a guard case.
Runs without a GPU: it reads declarations, it launches nothing."""

import os
import re

import test_gpu_guard_callback
import test_gpu_guard_packing
import test_gpu_guard_primitives

HERE = os.path.dirname(os.path.abspath(__file__))

# test_gpu_guard.py drives these through _nd.fused_encode_into / fused_decode_into
FUSED = {'kmp_volume_encode', 'kmp_volume_decode', 'kmp_image_encode', 'kmp_image_decode'}

# pure host queries: no launch, no device write
HOST = {'kmp_version', 'kmp_last_error', 'kmp_last_launch', 'kmp_device_ok', 'kmp_set_option', 'kmp_clear_option',
        'kmp_get_option', 'kmp_host_device_pointer', 'kmp_volume_workspace_bytes', 'kmp_image_workspace_bytes',
        'kmp_linear_moments_workspace_bytes', 'kmp_pack_blocks', 'kmp_pack_workspace_bytes', 'kmp_pack_total_offset',
        'kmp_rice_tiles', 'kmp_rice_bundle_workspace_bytes'}

# device writers guarded elsewhere: {entry point: (test module, test, why that is enough)}
EXEMPT = {
    'kmp_rice_bundle_decode_ranges': ('test_gpu_rice_ranges.py', 'test_guarded_outputs',
                                      'outputs of exactly end - first samples between sentinel guards, resident '
                                      'bundle and windows, vs the oracle'),
    'kmp_rice_tile_crc': ('test_gpu_tile_crc.py', 'test_windows_give_the_same_values_and_write_nothing_else',
                          'the CRC table between sentinel guards at aligned and misaligned windows, vs the spec'),
}

MODULES = (test_gpu_guard_primitives, test_gpu_guard_callback, test_gpu_guard_packing)


def _exported():
    from kompressor_amd import _lib
    return set(_lib.EXPORTED)


def test_every_device_writer_has_a_guard_case():
    launched = set()
    for m in MODULES:
        assert len(set(m.LAUNCHES)) == len(m.LAUNCHES)
        launched |= set(m.LAUNCHES)
    exported = _exported()
    groups = {'fused': FUSED, 'host': HOST, 'exempt': set(EXEMPT), 'launched': launched}
    names = list(groups)
    for i, a in enumerate(names):  # one place per function
        for b in names[i + 1:]:
            assert not groups[a] & groups[b], f'{sorted(groups[a] & groups[b])} listed as {a} and as {b}'
    listed = set().union(*groups.values())
    assert not listed - exported, f'listed but not exported by the library: {sorted(listed - exported)}'
    assert not exported - listed, ('exported without a guard case (add one to a test_gpu_guard_* module, or an '
                                   f'exemption with its reason): {sorted(exported - listed)}')


def test_the_header_declares_what_the_library_exports():
    """The ledger is built from ``_lib.EXPORTED``; this ties that list to the header's prototypes."""
    with open(os.path.join(HERE, '..', 'include', 'kompressor_hip.h')) as f:
        text = re.sub(r'/\*.*?\*/', ' ', f.read(), flags=re.S)
    declared = set(re.findall(r'\b(kmp_[a-z0-9_]+)\s*\(', text))
    assert declared == _exported()


def test_declared_launches_are_made_by_their_module():
    """Each declared entry point is named in a K.launch call of the module that declares it, and every
    module ends with the test that they all ran."""
    for m in MODULES:
        with open(m.__file__) as f:
            src = f.read()
        called = set(re.findall(r"K\.launch\(\s*'(kmp_[a-z0-9_]+)'", src))
        called |= {e + '_typed' for e in called if f"'{e}' + suffix" in src}
        called |= set(re.findall(r"\('(kmp_[a-z0-9_]+)', \(", src))  # (entry, extra arguments, ...) variant tables
        assert set(m.LAUNCHES) <= called, f'{m.__name__}: declared but not launched: {sorted(set(m.LAUNCHES) - called)}'
        assert hasattr(m, 'test_every_declared_entry_point_was_launched')


def test_exemptions_name_existing_tests():
    for entry, (module, test, reason) in EXEMPT.items():
        with open(os.path.join(HERE, module)) as f:
            src = f.read()
        assert f'def {test}(' in src and reason, f'{entry}: {module}::{test} does not exist'
        assert entry in src, f'{module} does not name {entry}'
