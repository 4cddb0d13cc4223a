"""Self-describing compressed files ("on-disk format + entropy coding").

The reference has no file format -- ``encode`` returns ``(lowres, (maps, dims))`` in memory
(volume/encode_decode.py:56) -- so this is the build's own container: one file holds the
entropy-coded ``encode`` result (``packing.pack_encoded``: block-adaptive Rice by default) plus
everything needed to decode it without outside knowledge -- the pyramid levels (``compress``
applies the reference's single-level ``encode`` recursively to the lowres, so only the coarsest
lowres is stored raw), the spatial rank, the predictor
(kind, padding, and a LinearPredictor's weights), the coder, the even-size ``dims``, the original
sample dtype (float32 volumes travel bit-cast to uint32) and a CRC-32 of the payload.

    info = compress(path, highres, predictor)     # pyramid encode on the GPU + Rice + one write
    highres = decompress(path)                    # read + unpack + decode on the GPU
    info = compress(path, highres, predictor, target_bits=4)   # the finest bound that fits 4 bits per sample
    size = compressed_size(highres, predictor, abs_error=1e-3)  # what compress would write, sized on the GPU
    save(path, lowres, encoded, predictor=...)    # an encode() result you already have
    lowres, encoded, meta = load(path)
    box = read_region(path, planes=(z0, z1), rows=(y0, y1), cols=(x0, x1), level=k)   # only the tiles the box needs
    shapes = level_shapes(path)                   # header + metadata only

File layout (little-endian): ``b'KMPF' u16 version u16 0 u64 meta_len``, the metadata as UTF-8
JSON padded to 8 bytes, then the ``pack_encoded`` bundle (``meta['bundle_bytes']`` bytes).  A file
written with ``tile_crc=True`` continues with zero bytes to an 8-byte boundary and a u32 table of
one CRC-32 per bundle tile (``meta['tile_crc'] = {'offset', 'tiles'}``, the offset from the bundle's
start; ``packing.tile_crcs``): ``read_region`` verifies the tiles it touches against it, ``check``
and a failing ``decompress`` name the damaged ones.  ``bundle_bytes`` and ``crc32`` cover the bundle
alone either way, and a reader that does not know the key reads the file as before.
Version 4 is a near-lossless file (``'max_error'``), version 5 an error-bounded float32 file
(``'quant'``, and its exception arrays behind the maps), version 6 a relative-error float32 file
(``'prec'``), version 7 either of the two with its exceptions stored as runs (``'exception_runs'``), version 8
a time series, delta-coded along the batch axis (``'temporal'``); see ``VERSION_NEAR`` / ``VERSION_QUANT`` /
``VERSION_PREC`` / ``VERSION_RUNS`` / ``VERSION_TEMPORAL`` below.

The host side of the file path (round 4): the bundle's CRC-32 (zlib's, the value the file stores)
is computed on the device (``kmp_crc32``) -- over the bundle the encode just wrote, its length read
by the kernel from the bundle header, so one synchronisation returns length and CRC together; on
read, over the bundle as uploaded, checked with the decode's side-information counter.  The bundle
crosses the link through a reused pinned staging buffer (57 GB/s instead of ~8 GB/s pageable) and
files are read straight into it; numpy results come back through the same pinned path
(``_device.to_host``).  ``last_timing`` holds the wall-time split of the last call.
"""

import json
import os
import struct
import time

import numpy as np
import torch

from . import _device as dev
from . import _nd, delta, metrics, near, packing, quant, rate
from ._lib import DECODE as _lib_decode, check as _check, coder_max_error as _lib_max_error, lib
from .predictors import ARITH_REV, LinearPredictor, MeanPredictor

# wall-time split (seconds) of the last compress / decompress / save / load of this process
last_timing = {}

MAGIC = b'KMPF'
VERSION = 3  # 2: rice payloads are v2 bundles (packing.py); 3: a LinearPredictor's arith_rev recorded
# 4: a near-lossless file: the metadata's 'max_error' > 0 is the bound its maps were
# quantised with.  Only such files carry it, so lossless files stay version 3, byte for byte, and a
# build from before near-lossless coding refuses a version-4 file instead of decoding it as lossless.
VERSION_NEAR = 4
# 5: an error-bounded float32 file: 'sample_dtype' is 'float32', the levels and the lowres
# are those of a lossless file of the int16 / int32 array ``quant.quantise`` made of it, and the metadata's
# 'quant' = {'exp', 'dtype', 'exceptions': E} records the step 2^exp, that integer dtype and the number
# of values kept as raw bits.  With E > 0 the bundle ends with three uint32 arrays of E entries: the low
# and the high words of the gaps between consecutive sorted flat indices (the first gap is the first
# index), and the bits.  Older builds refuse version 5.
VERSION_QUANT = 5
# 6: a relative-error float32 file: as version 5, but the integers are those of
# ``quant.quantise_rel`` and the metadata's 'prec' = {'bits', 'dtype', 'exceptions': E} records the
# mantissa bits kept in place of 'quant'.  The exception arrays are version 5's.  Older builds refuse it.
VERSION_PREC = 6
# 7: a version-5 or version-6 file whose exceptions are stored as runs (``exceptions='runs'``
# with E > 0): the metadata is that version's -- exactly one well-formed 'quant' or 'prec' -- plus
# 'exception_runs' = R, 1 <= R <= E; the integers under the exceptions are hold-filled, and the bundle ends
# with FOUR uint32 arrays of R entries (``quant.d_runs``): the low and high words of the gaps between
# consecutive run starts, the lengths, the differences of consecutive runs' bits modulo 2^32.  Older builds
# refuse version 7; with E == 0 the file is the version-5 / 6 one, byte for byte.
VERSION_RUNS = 7
# 8: a time series (``temporal='delta'``): the batch axis is time and the coded integers are the
# deltas ``kom.delta`` takes along it.  The metadata is that of the version the file would otherwise be (3, 5,
# 6 or 7: none, 'quant', 'prec', or one of them with 'exception_runs') plus 'temporal' = {'mode': 'delta',
# 'key_interval': K or 0 (only frame 0 is a key frame), 'dtype': the deltas' dtype -- the signed one of the
# samples' width, for a float32 file the quantiser's}.  The bundle's arrays are those of that version with the
# deltas in place of the integers.  Never a 'max_error'.  Older builds refuse version 8; without the keyword,
# and for a single frame, the file is the other version's byte for byte.
VERSION_TEMPORAL = 8
_TEMPORAL = (None, 'delta')
_TEMPORAL_DTYPES = {'int8': torch.int8, 'int16': torch.int16, 'int32': torch.int32}
_EXCEPTIONS = ('list', 'runs')
_QUANT_DTYPES ={'int16': torch.int16, 'int32': torch.int32}
_QUANT_SLAB = 1 << 24  # elements per slab of the bound's check
_HEAD = struct.Struct('<4sHHQ')
_NP_NAME = {torch.uint8: 'uint8', torch.uint16: 'uint16', torch.int32: 'int32', torch.uint32: 'uint32',
            torch.float32: 'float32', torch.int8: 'int8', torch.int16: 'int16'}
# Signed samples (int8 / int16): the metadata says 'int8' / 'int16' and the bundle stores the coarsest
# lowres under the signed dtype code, as its own bit pattern (the Rice zigzag reads samples as signed,
# so small signed values stay small); the maps are the unsigned residuals.  A build from before
# signed samples knows neither the name nor the code and refuses such a file.
_SAMPLE_NAMES = frozenset(_NP_NAME.values())


def _check_sample_dtype(meta, path):
    """A file of a sample dtype this build does not know is refused, not misdecoded."""
    for key in ('sample_dtype', 'lowres_dtype'):
        name = meta.get(key)
        if name is not None and name not in _SAMPLE_NAMES:
            raise ValueError(f'{path}: {key} {name!r} is not a sample dtype this build knows '
                             f'({", ".join(sorted(_SAMPLE_NAMES))}): read it with the build that wrote it')


def _check_max_error(meta, version, path):
    """A version-4 file states its bound, in range for its sample dtype; no other version has one."""
    delta = meta.get('max_error') if isinstance(meta, dict) else None
    if version != VERSION_NEAR:
        if delta not in (None, 0) or isinstance(delta, bool):
            raise ValueError(f'{path}: a version-{version} file with max_error {delta!r} (near-lossless files are '
                             f'version {VERSION_NEAR})')
        return
    name = meta.get('sample_dtype') or meta.get('lowres_dtype')
    try:
        if isinstance(delta, bool) or not isinstance(delta, int) or delta < 1:
            raise ValueError(f'max_error {delta!r}')
        near.check_max_error(name, delta)
    except (ValueError, TypeError) as e:
        raise ValueError(f'{path}: a version-{VERSION_NEAR} (near-lossless) file with a bad bound for {name!r} '
                         f'samples: {e}') from None


def _check_quant(meta, version, path):
    """A version-5 file is float32, states a well-formed 'quant' and carries no 'max_error'; no other
    version has a 'quant'."""
    q = meta.get('quant')
    if version != VERSION_QUANT:
        if q is not None:
            raise ValueError(f'{path}: a version-{version} file with a quant entry (error-bounded files are version '
                             f'{VERSION_QUANT})')
        return
    if 'max_error' in meta:
        raise ValueError(f'{path}: a version-{VERSION_QUANT} (error-bounded) file with a max_error entry')

    def is_int(v):
        return isinstance(v, int) and not isinstance(v, bool)
    if not (isinstance(q, dict) and is_int(q.get('exp')) and quant.E_MIN <= q['exp'] <= quant.E_MAX and
            isinstance(q.get('dtype'), str) and q['dtype'] in _QUANT_DTYPES and
            is_int(q.get('exceptions')) and q['exceptions'] >= 0):
        raise ValueError(f'{path}: a version-{VERSION_QUANT} (error-bounded) file with a bad quant entry {q!r}')
    if meta.get('sample_dtype') != 'float32':
        raise ValueError(f'{path}: a version-{VERSION_QUANT} (error-bounded) file of {meta.get("sample_dtype")!r} '
                         f'samples (float32 only)')


def _check_prec(meta, version, path):
    """A version-6 file is float32, states a well-formed 'prec' and carries neither 'quant' nor
    'max_error'; no other version has a 'prec'."""
    p = meta.get('prec')
    if version != VERSION_PREC:
        if p is not None:
            raise ValueError(f'{path}: a version-{version} file with a prec entry (relative-error files are version '
                             f'{VERSION_PREC})')
        return
    for key in ('max_error', 'quant'):
        if key in meta:
            raise ValueError(f'{path}: a version-{VERSION_PREC} (relative-error) file with a {key} entry')

    def is_int(v):
        return isinstance(v, int) and not isinstance(v, bool)
    if not (isinstance(p, dict) and is_int(p.get('bits')) and quant.M_MIN <= p['bits'] <= quant.M_MAX and
            isinstance(p.get('dtype'), str) and p['dtype'] in _QUANT_DTYPES and
            is_int(p.get('exceptions')) and p['exceptions'] >= 0):
        raise ValueError(f'{path}: a version-{VERSION_PREC} (relative-error) file with a bad prec entry {p!r}')
    if meta.get('sample_dtype') != 'float32':
        raise ValueError(f'{path}: a version-{VERSION_PREC} (relative-error) file of {meta.get("sample_dtype")!r} '
                         f'samples (float32 only)')


def _check_runs(meta, version, path):
    """The version whose rules the rest of the metadata follows.  A version-7 file carries exactly one of
    'quant' / 'prec' (checked as version 5 / 6 by the caller) and a well-formed 'exception_runs' R with
    1 <= R <= E; no other version has an 'exception_runs'."""
    if version != VERSION_RUNS:
        if 'exception_runs' in meta:
            raise ValueError(f'{path}: a version-{version} file with an exception_runs entry (files with exception '
                             f'runs are version {VERSION_RUNS})')
        return version
    if ('quant' in meta) == ('prec' in meta):
        raise ValueError(f'{path}: a version-{VERSION_RUNS} (exception runs) file needs exactly one of quant and prec')
    base = VERSION_QUANT if 'quant' in meta else VERSION_PREC
    (_check_quant if base == VERSION_QUANT else _check_prec)(meta, base, path)
    R, E = meta.get('exception_runs'), meta['quant' if base == VERSION_QUANT else 'prec']['exceptions']
    if isinstance(R, bool) or not isinstance(R, int) or not 1 <= R <= E:
        raise ValueError(f'{path}: a version-{VERSION_RUNS} (exception runs) file with a bad exception_runs entry '
                         f'{R!r} ({E} exceptions)')
    return base


def _check_temporal(meta, version, path):
    """The version whose rules the rest of the metadata follows.  A version-8 file carries a well-formed
    'temporal' and no 'max_error'; the rest is a version-3, -5, -6 or -7 file's, told apart by its 'quant',
    'prec' and 'exception_runs' entries.  No other version has a 'temporal'."""
    t = meta.get('temporal') if isinstance(meta, dict) else None
    if version != VERSION_TEMPORAL:
        if isinstance(meta, dict) and 'temporal' in meta:
            raise ValueError(f'{path}: a version-{version} file with a temporal entry (time series are version '
                             f'{VERSION_TEMPORAL})')
        return version
    if 'max_error' in meta:
        raise ValueError(f'{path}: a version-{VERSION_TEMPORAL} (time series) file with a max_error entry')
    K = t.get('key_interval') if isinstance(t, dict) else None
    if not (isinstance(t, dict) and t.get('mode') == 'delta' and isinstance(K, int) and not isinstance(K, bool) and
            K >= 0 and isinstance(t.get('dtype'), str) and t['dtype'] in _TEMPORAL_DTYPES):
        raise ValueError(f'{path}: a version-{VERSION_TEMPORAL} (time series) file with a bad temporal entry {t!r}')
    if 'exception_runs' in meta:
        base = VERSION_RUNS
    else:
        base = VERSION_QUANT if 'quant' in meta else VERSION_PREC if 'prec' in meta else VERSION
    q = meta.get('quant') or meta.get('prec')
    name = q.get('dtype') if isinstance(q, dict) else meta.get('sample_dtype')
    want = _NP_NAME.get(delta.SIGNED.get(delta.NAMES.get(name)))
    if t['dtype'] != want:
        raise ValueError(f'{path}: a version-{VERSION_TEMPORAL} (time series) file whose deltas are {t["dtype"]!r}: '
                         f'those of {name!r} values are {want!r}')
    return base


def _temporal(meta):
    """``(K or None, the deltas' torch dtype)`` of a time series whose header ``_read_head`` accepted, else None."""
    t = meta.get('temporal')
    if t is None:
        return None
    return (int(t['key_interval']) or None), _TEMPORAL_DTYPES[t['dtype']]


def _versioned(meta, version):
    """The version a file of ``meta`` is written as: ``version``, or 8 for a time series."""
    return VERSION_TEMPORAL if 'temporal' in meta else version


def _runs(meta):
    """R of a file whose header ``_read_head`` accepted and that stores its exceptions as runs, else 0."""
    return int(meta.get('exception_runs') or 0)


def _quant(meta):
    """``(exp or kept mantissa bits, torch dtype, E, the restoring function)`` of an error-bounded
    ('quant') or relative-error ('prec') file whose header ``_read_head`` accepted, else None."""
    for key, param, d_restore in (('quant', 'exp', quant.d_restore), ('prec', 'bits', quant.d_restore_rel)):
        q = meta.get(key)
        if q is not None:
            return int(q[param]), _QUANT_DTYPES[q['dtype']], int(q['exceptions']), d_restore
    return None


def _max_error(meta):
    """The bound of a file whose header ``_read_head`` accepted (0: lossless)."""
    return int(meta.get('max_error') or 0)


def _predictor_meta(predictor, padding, ndim, dtype):
    """(``dtype``: the coded samples' torch dtype -- a LinearPredictor's arithmetic is recorded
    resolved for it, so a reader needs no rule for ``'auto'``)"""
    if isinstance(predictor, MeanPredictor):
        return {'kind': 'mean', 'padding': predictor.padding, 'ndim': predictor.ndim}
    if isinstance(predictor, LinearPredictor):
        return {'kind': 'linear', 'padding': predictor.padding, 'ndim': predictor.ndim,
                'arith': predictor.arith_for(dtype), 'arith_rev': ARITH_REV[predictor.arith_for(dtype)],
                'weights': predictor.weights.tolist(), 'bias': predictor.bias.tolist()}
    # an opaque predictions_fn: recorded by name; decoding needs the caller to pass it again
    return {'kind': 'external', 'padding': padding, 'ndim': ndim,
            'name': getattr(predictor, '__qualname__', type(predictor).__name__)}


def predictor_from_meta(meta):
    """The built-in predictor a file was coded with (None for an external predictions_fn)."""
    p = meta['predictor']
    if p['kind'] == 'mean':
        return MeanPredictor(p['padding'], p['ndim'])
    if p['kind'] == 'linear':
        _check_arith_rev(meta)
        return LinearPredictor(np.asarray(p['weights'], np.float32), np.asarray(p['bias'], np.float32),
                               p['padding'], p['ndim'], p.get('arith', 'f32'))
    return None


def _check_arith_rev(meta, path='file'):
    """A LinearPredictor file decodes only under the arithmetic revision it was coded with
    (predictors.ARITH_REV): a different revision rounds some predictions differently and would
    return wrong samples.  Files before container version 3 carry no revision; their f32 chain is
    revision 1, their bf16x2 data is ambiguous (round 4 and round 5 builds wrote it with different
    accumulation orders) and is refused."""
    p = meta.get('predictor') or {}
    if p.get('kind') != 'linear':
        return
    arith = p.get('arith', 'f32')
    rev = p.get('arith_rev', 1 if arith == 'f32' else None)
    if arith not in ARITH_REV:
        raise ValueError(f"{path}: unknown LinearPredictor arithmetic {arith!r}")
    if rev != ARITH_REV[arith]:
        raise ValueError(f"{path}: coded with arith={arith!r} revision {rev if rev is not None else 'unrecorded'}; "
                         f"this build evaluates revision {ARITH_REV[arith]}, whose rounding differs -- decode it "
                         f"with the build that wrote it")


def _device_crc(blob, n_max, n_dev=None):
    """zlib CRC-32 of the device bytes ``blob[:n]`` (n = ``n_max``, or the device int64 at ``n_dev``
    capped to ``n_max``) as a 1-element device uint32 tensor; no synchronisation."""
    out = torch.empty((1,), dtype=torch.int32, device='cuda')
    _check(lib.kmp_crc32(blob.data_ptr(), int(n_max), n_dev, out.data_ptr(), dev.stream()), 'crc32')
    return out


def _bundle(x, arrays, dims, method, tile_crc=False):
    """Entropy-code an encode result on the device: ``(device bytes, bundle length, crc32, per-tile
    CRC table bytes or None)`` with ONE synchronisation (length, CRC and -- ``tile_crc`` -- the table,
    computed by ``kmp_rice_tile_crc`` on the same stream right after the encode, read back together)."""
    if method == 'rice':
        out, poff, launched, keep = packing._rice_encode_launch((x, *arrays), dims)
        T = 0
        if tile_crc and launched:
            plan = packing._rice_enc_plan(keep, dims)
            T = plan['T']
            table = torch.empty((T,), dtype=torch.int32, device='cuda')
            # the payload's extent is not known on the host yet: the spans are checked against the buffer
            packing._launch_tile_crc(packing._resident_crc_records(
                out.data_ptr(), plan['ns'], plan['offs'], poff, (out.numel() - poff) // 4, table.data_ptr()), None)
        head = dev.pinned_staging(64 + 4 * T, 'head')
        if not launched:  # no samples: the header and side arrays only
            total = poff
            crc = _device_crc(out, total)
            head[:4].copy_(crc.view(torch.uint8), non_blocking=True)
        else:
            crc = _device_crc(out, out.numel(), out[64:72].data_ptr())  # the size field of the header
            head[:16].copy_(out[56:72], non_blocking=True)
            head[16:20].copy_(crc.view(torch.uint8), non_blocking=True)
            if T:
                head[64:64 + 4 * T].copy_(table.view(torch.uint8), non_blocking=True)
        torch.cuda.current_stream().synchronize()
        hb = head[:20].numpy().tobytes()
        tab = head[64:64 + 4 * T].numpy().tobytes() if tile_crc else None
        del keep
        if launched:
            _, total = struct.unpack('<2q', hb[:16])
            return out, int(total), struct.unpack('<I', hb[16:20])[0], tab
        return out, int(total), struct.unpack('<I', hb[:4])[0], tab
    if tile_crc:
        raise ValueError("tile_crc=True needs method='rice' (a 'planes' bundle has no tiles)")
    blob = packing.pack_encoded(x, (arrays, dims), method)
    crc = _device_crc(blob, blob.numel())
    return blob, blob.numel(), int(crc.cpu().view(torch.uint32).item()), None


def _meta_bytes(meta, total, crc, tiles=None):
    """The metadata as a file stores it: ``meta`` plus the bundle's length and CRC-32 (and, for a file
    with a per-tile CRC table of ``tiles`` entries, where it lies), compact JSON padded to 8 bytes."""
    meta = dict(meta, bundle_bytes=int(total), crc32=int(crc) & 0xffffffff)
    if tiles is not None:
        meta['tile_crc'] = {'offset': int(total) + (-int(total) % 8), 'tiles': int(tiles)}
    js = json.dumps(meta, separators=(',', ':')).encode()
    return js + b' ' * (-len(js) % 8)


def _bound_bytes(meta, total, tiles=None):
    """``bound_bytes``: the length of the file of ``meta`` and a bundle of ``total`` bytes (``tiles``: its
    per-tile CRC table's entries, None without one) with the widest CRC-32, 4294967295.  The CRC is
    stored as a decimal, so the file written is never larger than this and at most 16 bytes smaller."""
    trailer = 0 if tiles is None else (-int(total) % 8) + 4 * int(tiles)
    return _HEAD.size + len(_meta_bytes(meta, total, 0xffffffff, tiles)) + int(total) + trailer


def _write(path, meta, blob, total, crc, t0, table=None, version=VERSION):
    """Header, metadata and the first ``total`` device bytes of ``blob`` to ``path``: the bundle
    crosses the link in pinned chunks (``_device.d2h_stream``), each written to the file while the
    next ones are in flight.  ``table`` (the per-tile CRCs, u32 little-endian) follows the bundle,
    8-aligned, and is recorded in the metadata as ``'tile_crc': {'offset', 'tiles'}``."""
    t1 = time.perf_counter()
    trailer = b''
    if table is not None:
        trailer = b'\0' * (-int(total) % 8) + table
    js = _meta_bytes(meta, total, crc, None if table is None else len(table) // 4)
    tmp = f'{path}.tmp{os.getpid()}'
    with open(tmp, 'wb') as f:
        try:  # the file's blocks allocated up front: the write then only copies (8.0 vs 10.0 ms for
            os.posix_fallocate(f.fileno(), 0, _HEAD.size + len(js) + total + len(trailer))  # 112 MB, write_probe_r5w2.log)
        except OSError:
            pass  # a filesystem without fallocate: the writes allocate
        f.write(_HEAD.pack(MAGIC, version, 0, len(js)))
        f.write(js)
        if total:
            dev.d2h_stream(blob[:total], lambda lo, piece: f.write(memoryview(piece)))
        f.write(trailer)
    os.replace(tmp, path)  # a reader never sees a half-written file
    t2 = time.perf_counter()
    last_timing.clear()
    last_timing.update(device=t1 - t0, d2h_write=t2 - t1, total=t2 - t0)
    return _HEAD.size + len(js) + total + len(trailer)


def _builtin_padding(predictor, padding):
    """The padding a file records: a built-in predictor carries its own (a conflicting explicit
    ``padding`` is an error); an external predictions_fn needs it passed (default 0)."""
    if isinstance(predictor, (MeanPredictor, LinearPredictor)):
        if padding is not None and int(padding) != predictor.padding:
            raise AssertionError(f'padding={padding} conflicts with the predictor\'s padding {predictor.padding}')
        return predictor.padding
    return 0 if padding is None else int(padding)


def _check_tile_crc_method(tile_crc, method):
    if tile_crc and method != 'rice':
        raise ValueError("tile_crc=True needs method='rice' (a 'planes' bundle has no tiles)")


def save(path, lowres, encoded, predictor=None, padding=None, ndim=None, method='rice', sample_dtype=None,
         tile_crc=False, max_error=0):
    """Write an ``encode`` result ``(lowres, (maps, dims))`` to ``path``; returns the file size.
    ``predictor`` is recorded so :func:`decompress` can decode without being told.  ``padding``
    defaults to a built-in predictor's own padding (0 for an external predictions_fn).
    ``tile_crc=True`` (``method='rice'``) appends the per-tile CRC table :func:`read_region` checks
    the tiles it touches against.  ``max_error > 0``: ``encoded`` was made with
    ``near.coders(dtype, max_error)``; the bound is recorded and the file is version 4 (the samples
    are not at hand here, so the bound itself is checked where they are: :func:`compress`, or the
    caller's own decode)."""
    maps, dims = encoded
    ndim = ndim or len(dims)
    padding = _builtin_padding(predictor, padding)
    near.check_max_error(near._input_dtype(lowres), max_error)  # before the device is touched
    t0 = time.perf_counter()
    packing._check_method(method)
    _check_tile_crc_method(tile_crc, method)
    lo_t = dev.to_device(lowres)[0]
    maps_t = [dev.to_device(m)[0] for m in maps]
    if max_error:
        want = _nd.CODER_DTYPE[near.coder_id(lo_t.dtype, max_error)]
        if any(m.dtype != want for m in maps_t):
            raise TypeError(f'near-lossless maps of {lo_t.dtype} samples are {want}')
    meta = {'format': 'kompressor_amd', 'ndim': ndim, 'padding': padding, 'dims': [int(d) for d in dims],
            'method': method, 'lowres_shape': list(lo_t.shape), 'lowres_dtype': _NP_NAME[lo_t.dtype],
            'map_dtype': _NP_NAME[maps_t[0].dtype],
            'sample_dtype': sample_dtype or _NP_NAME[lo_t.dtype],
            'predictor': _predictor_meta(predictor, padding, ndim, lo_t.dtype) if predictor is not None else None}
    if max_error:
        meta['max_error'] = int(max_error)
    blob, total, crc, table = _bundle(lo_t, maps_t, dims, method, tile_crc)
    return _write(path, meta, blob, total, crc, t0, table, VERSION_NEAR if max_error else VERSION)


def _read_head(f, path):
    """``(version, meta, metadata bytes, bundle bytes)`` of the open file ``f``: the header and the
    metadata JSON, checked, with the bundle's recorded length checked against the file's size."""
    head = f.read(_HEAD.size)
    if len(head) < _HEAD.size:
        raise ValueError(f'{path}: not a kompressor_amd file (too short)')
    magic, version, _, mlen = _HEAD.unpack(head)
    if magic != MAGIC or version not in (1, 2, VERSION, VERSION_NEAR, VERSION_QUANT, VERSION_PREC, VERSION_RUNS,
                                         VERSION_TEMPORAL) or mlen > (1 << 26):
        raise ValueError(f'{path}: not a kompressor_amd file (magic {magic!r}, version {version})')
    try:
        meta = json.loads(f.read(mlen).decode())
        n = int(meta['bundle_bytes'])
    except (ValueError, KeyError, TypeError) as e:
        raise ValueError(f'{path}: corrupt metadata ({e})') from None
    _check_sample_dtype(meta, path)
    base = _check_temporal(meta, version, path)  # a version-8 file follows version 3's, 5's, 6's or 7's rules
    base = _check_runs(meta, base, path)  # a version-7 file follows version 5's or 6's rules
    _check_max_error(meta, base, path)
    _check_quant(meta, base, path)
    _check_prec(meta, base, path)
    if version == 1 and meta.get('method') != 'planes':
        # version-1 'rice' payloads were the per-array KMPR format, replaced by the v2 bundle;
        # version-1 'planes' payloads are unchanged and still read
        raise ValueError(f'{path}: a version-1 rice file (the retired per-array KMPR format): re-compress it')
    # the payload length is checked against the file before anything is allocated for it
    avail = os.fstat(f.fileno()).st_size - (_HEAD.size + mlen)
    if not 0 <= n <= avail:
        raise ValueError(f'{path}: truncated or corrupt ({n} payload bytes recorded, {max(avail, 0)} present)')
    return version, meta, mlen, n


def _read(path):
    """``(meta, device bundle, device crc, timing)``: the file's bundle read straight into the pinned
    staging buffer, uploaded, and its CRC-32 launched on the device (checked by the caller together
    with the decode's own synchronisation -- ``_check_crc``)."""
    t0 = time.perf_counter()
    with open(path, 'rb') as f:
        version, meta, mlen, n = _read_head(f, path)
        # the payload: parallel page-cache reads into pinned chunks, each uploaded while the next is read
        blob = torch.empty((max(n, 1),), dtype=torch.uint8, device='cuda')[:n]
        fd, base = f.fileno(), _HEAD.size + mlen
        got = dev.h2d_stream(blob, lambda lo, piece: dev.pread_into(fd, piece, base + lo)) if n else 0
    if got != n:
        raise ValueError(f'{path}: truncated ({got} of {n} payload bytes)')
    t1 = time.perf_counter()
    crc = _device_crc(blob, n) if n else torch.zeros((1,), dtype=torch.int32, device='cuda')
    return meta, blob, crc, {'read_upload': t1 - t0, 't_upload': t1}


def _check_crc(path, meta, crc, blob=None):
    """The device CRC against the file's (one small read-back; the caller's own synchronisation
    usually has already drained the stream).  On a mismatch of a file that has a per-tile CRC table,
    ``blob`` (the resident bundle) is checked tile by tile and the message names the damaged
    ``(array, tile)`` pairs."""
    got = int(crc.cpu().view(torch.uint32).item()) if meta['bundle_bytes'] else 0
    if got != (int(meta['crc32']) & 0xffffffff):
        where = ''
        if blob is not None and meta.get('tile_crc') is not None:
            try:
                T, bad = _damaged_tiles(path, meta, blob)
                shown = ', '.join(f'({a}, {t})' for a, t in bad[:8])
                where = f': {len(bad)} of {T} tiles damaged, (array, tile) = {shown}{", ..." if len(bad) > 8 else ""}' \
                    if bad else f': all {T} tile CRCs match, the damage lies outside the tiles'
            except ValueError as e:  # the table or the bundle's layout is itself unusable
                where = f'; the per-tile CRC table could not be used ({e})'
        raise ValueError(f'{path}: payload CRC mismatch (corrupt file){where}')


def _damaged_tiles(path, meta, blob):
    """``(T, [(array, tile), ...])``: the tiles of the resident bundle ``blob`` whose CRC differs from
    the file's per-tile table (``kmp_rice_tile_crc`` over the whole bundle, one launch per 32 arrays,
    one read-back).  ValueError when the table or the bundle's layout cannot be used."""
    with open(path, 'rb') as f:
        _, _, mlen, n = _read_head(f, path)
        base = _HEAD.size + mlen
        off, T = _tile_crc_trailer(meta, n, os.fstat(f.fileno()).st_size - base, path)
        want = np.frombuffer(os.pread(f.fileno(), 4 * T, base + off), np.uint32)
    if want.size != T:
        raise ValueError(f'{path}: truncated per-tile CRC table')
    got = packing.tile_crcs(blob)
    if got.numel() != T:
        raise ValueError(f'{path}: the bundle holds {got.numel()} tiles, the per-tile CRC table {T}')
    got = got.view(torch.int32).cpu().numpy().view(np.uint32)
    _, _, plan = packing._resident_bundle(blob)
    begins = _tile_begins([_tiles(k) for k in plan['ns']])
    bad = []
    for g in np.flatnonzero(got != want):
        a = max(i for i, b in enumerate(begins) if b <= g)
        bad.append((int(a), int(g - begins[a])))
    return T, bad


def check(path):
    """Verify a file without decoding it: ``{'ok', 'crc32': whether the bundle's CRC-32 matches,
    'tile_crc': None for a file without a per-tile table, else {'tiles': T, 'bad': [(array, tile),
    ...]}}`` (``'error'`` added there when the table or the bundle's layout cannot be used).  Damage
    is reported, never raised; only a file whose header cannot be read raises ValueError."""
    meta, blob, crc, _ = _read(path)
    got = int(crc.cpu().view(torch.uint32).item()) if meta['bundle_bytes'] else 0
    crc_ok = got == (int(meta['crc32']) & 0xffffffff)
    tiles = None
    if meta.get('tile_crc') is not None:
        try:
            T, bad = _damaged_tiles(path, meta, blob)
            tiles = {'tiles': T, 'bad': bad}
        except ValueError as e:
            tc = meta['tile_crc']
            T = tc.get('tiles') if isinstance(tc, dict) else None
            tiles = {'tiles': T if isinstance(T, int) else 0, 'bad': [], 'error': str(e)}
    return {'ok': crc_ok and (tiles is None or (not tiles['bad'] and 'error' not in tiles)), 'crc32': crc_ok,
            'tile_crc': tiles}


def load(path, device=True):
    """``(lowres, (maps, dims), meta)`` from a file written by :func:`save` / :func:`compress`;
    device tensors by default, numpy arrays with ``device=False``."""
    meta, blob, crc, _ = _read(path)
    _check_crc(path, meta, crc, blob)  # before any header parsing of a possibly corrupt bundle
    lowres, (maps, dims) = packing.unpack_encoded(blob)
    if not device:
        lowres, maps = dev.to_host(lowres), tuple(dev.to_host(m) for m in maps)
    return lowres, (maps, dims), meta


def _auto_levels(shape, ndim, max_levels=4):
    """Pyramid levels while every spatial extent stays >= 3 (its lowres >= 2, volume/utils.py:295-303)."""
    sp, levels = list(shape[1:1 + ndim]), 0
    while levels < max_levels and all(s >= 3 for s in sp):
        sp = [(s + (s + 1) % 2 + 1) // 2 - (s + 1) % 2 for s in sp]  # the trimmed lowres extent
        levels += 1
    return max(levels, 1)


def _lossless_levels(h, predictor, levels):
    """The lossless pyramid of the device tensor ``h`` under its dtype's natural coder: ``(coarsest
    lowres, every level's maps finest first, the metadata's level entries, levels)``."""
    ndim = predictor.ndim
    coder = _nd.NATURAL_CODER.get(h.dtype)
    if coder is None:
        raise TypeError(f'no lossless coder for {h.dtype}')
    levels = _auto_levels(h.shape, ndim) if levels == 'auto' else int(levels)
    _nd._require(levels >= 1, 'levels must be >= 1')
    x, arrays, meta_levels = h, [], []
    for _ in range(levels):
        sp = _nd._sp(x.shape, ndim)
        _nd.validate_highres_shape((x.shape[0], *[s + (s + 1) % 2 for s in sp], *x.shape[1 + ndim:]), ndim)
        lowres, maps, dims = _nd._alloc_encoded(x, coder, ndim)
        _nd.fused_encode_into(x, predictor, coder, lowres, maps, ndim)
        arrays.extend(maps)
        meta_levels.append({'highres_shape': list(x.shape), 'dims': [int(d) for d in dims]})
        x = lowres
    return x, arrays, meta_levels, levels


def _check_bounds(highres, max_error, abs_error, rel_error):
    """The bounds of a ``compress`` / ``compressed_size`` call, checked before the device is touched:
    ``(exp or None, kept mantissa bits or None)``."""
    exp = bits = None
    if rel_error is not None:
        bits = quant.mantissa_bits(rel_error)
        if max_error or abs_error is not None:
            raise ValueError('max_error, abs_error and rel_error exclude each other')
        quant._require_f32(highres, 'compress(rel_error=...)')
    if abs_error is not None:
        exp = quant.exponent(abs_error)
        if max_error:
            raise ValueError('abs_error (float32 samples) and max_error (8- / 16-bit integer samples) exclude each other')
        quant._require_f32(highres, 'compress(abs_error=...)')
    near.check_max_error(near._input_dtype(highres), max_error)
    return exp, bits


def _check_exceptions(exceptions, abs_error, rel_error, mode=None):
    """The ``exceptions`` keyword of a ``compress`` / ``compressed_size`` call, checked on the host alone:
    whether the exceptions are stored as runs.  ValueError for a value other than 'list' / 'runs', and for
    'runs' without ``abs_error``, ``rel_error`` or a float32 target (only those files have exceptions)."""
    if not isinstance(exceptions, str) or exceptions not in _EXCEPTIONS:
        raise ValueError(f"exceptions must be 'list' or 'runs', got {exceptions!r}")
    if exceptions == 'runs' and abs_error is None and rel_error is None and mode not in ('abs', 'rel'):
        raise ValueError("exceptions='runs' needs abs_error, rel_error or a float32 target: no other file has exceptions")
    return exceptions == 'runs'


def _check_temporal_args(highres, temporal, key_interval, max_error, abs_error, rel_error, mode=None):
    """The ``temporal`` / ``key_interval`` keywords of a ``compress`` / ``compressed_size`` call, checked on the
    host alone: None, or ``(K or None,)`` for a time series.  ValueError for a ``temporal`` other than None /
    'delta', a ``key_interval`` without it or one that is a bool, no int or < 1, 'delta' with a near-lossless
    bound (a per-frame error would add up along the chain) and 'delta' for lossless float32 / uint32 samples."""
    if isinstance(temporal, (bool, bytes)) or temporal not in _TEMPORAL:
        raise ValueError(f"temporal must be None or 'delta', got {temporal!r}")
    if temporal is None:
        if key_interval is not None:
            raise ValueError("key_interval needs temporal='delta'")
        return None
    K = delta.check_key_interval(key_interval)
    if max_error or mode == 'near':
        raise ValueError("temporal='delta' does not go with max_error or a near-lossless target: the per-frame "
                         'errors would add up along the chain')
    if abs_error is None and rel_error is None and mode is None:
        try:
            delta.sample_dtype(near._input_dtype(highres), "compress(temporal='delta')")
        except TypeError as e:
            raise ValueError(f'{e} (float32 samples: with abs_error, rel_error or a target)') from None
    return (K,)


def _single_frame(tk, h):
    """``tk`` for the device tensor ``h``: a series of one frame (or none) is the ordinary file."""
    return tk if tk is not None and h.shape[0] > 1 else None


def compress(path, highres, predictor, levels='auto', method='rice', tile_crc=False, max_error=0, abs_error=None,
             rel_error=None, target_bits=None, target_ratio=None, target_mode=None, target_psnr=None, exceptions='list',
             temporal=None, key_interval=None, target_ssim=None):
    """Encode ``highres`` with a built-in ``predictor`` (:class:`MeanPredictor` /
    :class:`LinearPredictor`) and the lossless coder of its dtype (uint8 / uint16 modular, int8 / int16
    modular on the sign-mapped samples, int32 raw, float32 bit-cast to uint32 modulo 2^32) as a ``levels``-deep pyramid -- each level is the
    reference's single-level ``encode`` (volume/encode_decode.py:30-56) applied to the previous
    level's lowres, so only the coarsest lowres is stored raw -- entropy-code every array and write
    ``path``.  Returns ``{'bytes', 'raw_bytes', 'ratio', 'bits_per_sample', 'levels'}``.
    ``tile_crc=True`` (``method='rice'``) appends one CRC-32 per tile of 16384 samples, computed on the
    device right after the encode, so :func:`read_region` verifies exactly the tiles it reads.
    ``max_error = d > 0`` (uint8 / uint16 / int8 / int16 samples): near-lossless -- the closed loop of
    ``near.encode_pyramid``, every restored sample within ``d`` of the original, which is checked on
    the device before anything is written (a failed check raises and writes nothing); the file is
    version 4 and the result also holds ``'max_error'`` and the measured ``'max_abs_error'``.
    ``abs_error`` (float32 samples; not with ``max_error``): error-bounded -- ``quant.quantise`` under the
    bound, then the lossless pyramid of the int16 / int32 array; every restored value is within
    ``quant.effective(abs_error)`` of the original and the values that cannot be quantised (not finite,
    out of the integer range) come back bit for bit.  The bound is checked on the device before
    anything is written; the file is version 5 and the result also holds ``'abs_error'`` (the effective
    bound), ``'abs_error_asked'``, ``'max_abs_error'``, ``'exceptions'`` and ``'quant_dtype'``.
    ``rel_error`` (float32 samples; alone of the three bounds): pointwise relative -- ``quant.quantise_rel``,
    then the same pyramid; every restored value ``r`` of a finite ``x`` has ``|r - x| <=
    quant.effective_rel(rel_error) * max(|x|, 2**-126)``, what is not finite or rounds up to infinity
    comes back bit for bit.  Checked on the device before anything is written; the file is version 6
    and the result also holds ``'rel_error'`` (the effective bound), ``'rel_error_asked'``,
    ``'max_rel_error'``, ``'exceptions'`` and ``'quant_dtype'``.
    ``target_bits`` (bits per sample of the whole file) or ``target_ratio`` (raw bytes / file bytes), one of
    them and none of the three bounds, ``method='rice'``: rate control (``kompressor_amd.rate``, DESIGN.md
    §19) -- the finest bound of a ladder whose file fits ``floor(target_bits * numel / 8)`` or
    ``floor(raw_bytes / target_ratio)`` bytes.  ``target_mode``: ``'abs'`` (default) or ``'rel'`` for
    float32 samples, ``'near'`` for uint8 / uint16 / int8 / int16.  Each candidate is sized on the device
    by :func:`compressed_size`; the chosen one is then written by the explicit-bound path above, so the
    file is byte for byte that of ``abs_error = 2**(e - 1)`` / ``rel_error = 2**-(m + 1)`` /
    ``max_error = d``, and the result is that call's plus ``'target_bytes'`` (the budget),
    ``'bound_bytes'`` and ``'probes'`` (``[(e or m or d, bound_bytes), ...]`` in the order asked).  A
    budget below the coarsest rung raises ValueError and writes nothing.
    ``target_psnr`` (dB; alone of the targets and bounds, any ``method``): a quality target --
    the COARSEST bound of the same ladders (``target_mode`` as above) whose PSNR, measured on the device
    against the value range (float32) or ``2^W - 1`` (integer samples), is at least the target; a probe is
    the quantiser (or the closed loop) and the comparing launch, no pyramid and no sizing for float32.
    The chosen rung is written by the explicit-bound path, so the file is byte for byte that call's and
    the result is that call's plus ``'target_psnr'`` and ``'probes'`` (``[(e or m or d, psnr), ...]`` in the
    order asked).  A target above the finest rung's PSNR raises ValueError and writes nothing.
    ``target_ssim`` (``0 < s <= 1``; alone of the targets and bounds, any ``method``): a structural quality target
     -- the COARSEST bound of the same ladders whose mean SSIM (``metrics.ssim``: 7-sample windows
    inside each item, the default peak, float32 samples shifted by the smallest finite value) is at least the
    target.  Peak, base and the ladder are fixed once from one comparison of the array with itself.  A float32
    probe is the quantiser, the WHOLE array restored with its exceptions put back (one more array of device
    memory than ``target_psnr``'s slabs: a window spans slabs) and one SSIM call; a ``'near'`` probe is the closed
    loop and one SSIM call, and the lossless rung 0 is 1.0 without a launch.  The chosen rung is written by the
    explicit-bound path, so the file is byte for byte that call's (no new version, no new metadata) and the
    result is that call's plus ``'ssim'`` (the chosen rung's), ``'target_ssim'`` and ``'probes'`` (``[(e or m or d,
    ssim), ...]``).  A target above the finest rung's SSIM raises ValueError and writes nothing; so do a
    spatial extent below 7 (before the device is touched) and a float32 array whose finite values span no range.
    Quality figures: every lossy result also holds ``'mse'``, ``'psnr'`` and ``'value_range'``, measured by
    ``kom.metrics`` on exactly what :func:`decompress` returns (NaNs and infinities, which come back bit for
    bit, are not compared); a lossless one holds ``'mse': 0.0`` and ``'psnr': inf``.
    ``exceptions='runs'`` (with ``abs_error``, ``rel_error`` or a float32 target): for masked fields --
    the values that cannot be quantised are stored as runs of consecutive indices with equal bits
    (``quant.runs``) instead of one index and 32 bits each, and the integers under them are hold-filled
    (``quant.fill``) so that a hole costs the pyramid next to nothing.  What :func:`decompress` returns is bit
    for bit what the ``'list'`` file returns.  With exceptions the file is version 7; without any it is the
    ``'list'`` file byte for byte.  The result also holds ``'exception_runs'``.
    ``temporal='delta'`` (not with ``max_error`` or a near-lossless target, not for lossless
    float32 / uint32 samples): a time series -- the batch axis is time and every frame but the key frames is
    coded as its difference from the frame before it, modulo 2^W, on the integers (``kom.delta``: the
    samples of a lossless file, for a float32 file the quantiser's integers after marks and fill), then the
    unchanged pyramid.  ``key_interval = K``: frame ``t`` is a key frame iff ``t % K == 0``; None: frame 0 alone
    (``key_interval`` without ``temporal`` is ValueError).  What :func:`decompress` returns is bit for bit what
    the same call without ``temporal`` returns, and every bound is checked on exactly that; ``read_region``
    of frames ``a .. b`` decodes from the key frame at or before ``a``.  The file is version 8 and the result
    also holds ``'temporal'`` and ``'key_interval'``; a single frame writes the ordinary file, byte for byte."""
    mode = rate.check_target(near._input_dtype(highres), target_bits, target_ratio, target_mode, method, max_error,
                             abs_error, rel_error, target_psnr, target_ssim)  # before the device is touched
    if target_ssim is not None:
        metrics.ssim_dims(highres.shape, 'compress(target_ssim=...)')  # likewise
    exp, bits = _check_bounds(highres, max_error, abs_error, rel_error)  # before the device is touched
    runs = _check_exceptions(exceptions, abs_error, rel_error, mode)  # before the device is touched
    tk = _check_temporal_args(highres, temporal, key_interval, max_error, abs_error, rel_error, mode)  # likewise
    t0 = time.perf_counter()
    packing._check_method(method)
    _check_tile_crc_method(tile_crc, method)
    h, _ = dev.to_device(highres)
    tk = _single_frame(tk, h)
    if target_psnr is not None:
        return _compress_psnr(path, h, predictor, levels, method, tile_crc, mode, float(target_psnr), t0, runs, tk)
    if target_ssim is not None:
        return _compress_ssim(path, h, predictor, levels, method, tile_crc, mode, float(target_ssim), t0, runs, tk)
    if mode is not None:
        return _compress_target(path, h, predictor, levels, tile_crc, mode, target_bits, target_ratio, t0, runs, tk)
    if max_error:
        return _compress_near(path, h, predictor, levels, method, tile_crc, int(max_error), t0)
    if exp is not None:
        return _compress_quant(path, h, predictor, levels, method, tile_crc, abs_error, exp, t0, runs, tk)
    if bits is not None:
        return _compress_prec(path, h, predictor, levels, method, tile_crc, rel_error, bits, t0, runs, tk)
    return _compress_lossless(path, h, predictor, levels, method, tile_crc, t0, tk)


def _temporal_meta(tk, d):
    """The metadata's 'temporal' entry of the deltas ``d`` taken under ``tk``."""
    return {'mode': 'delta', 'key_interval': tk[0] or 0, 'dtype': _NP_NAME[d.dtype]}


def _temporal_result(tk):
    """What a :func:`compress` result says of a time series."""
    return {} if tk is None else {'temporal': 'delta', 'key_interval': tk[0]}


def _compress_lossless(path, h, predictor, levels, method, tile_crc, t0, tk=None):
    """:func:`compress` without a bound: the lossless pyramid, the version-3 file (``tk``: of the deltas along
    the batch axis, the version-8 file)."""
    p = _parts_lossless(h, predictor, levels, method, tk)
    blob, total, crc, table = _bundle(p['x'], p['arrays'], (), method, tile_crc)
    nbytes = _write(path, p['meta'], blob, total, crc, t0, table, _versioned(p['meta'], VERSION))
    raw = h.numel() * h.element_size()
    return {'bytes': nbytes, 'raw_bytes': raw, 'ratio': raw / nbytes, 'bits_per_sample': 8.0 * nbytes / h.numel(),
            'levels': p['levels'], 'max_error': 0, 'max_abs_error': 0, 'mse': 0.0, 'psnr': float('inf'),
            **_temporal_result(tk)}


# The arrays and the metadata of a file, before anything is entropy-coded: what :func:`compress` bundles
# and writes and what :func:`compressed_size` only measures.  Each returns {'x': the coarsest lowres,
# 'arrays': the bundle's arrays after it, 'meta', 'levels'} and its mode's own entries.

def _parts_lossless(h, predictor, levels, method, tk=None):
    ndim, padding = predictor.ndim, predictor.padding
    sample = _NP_NAME[h.dtype]
    if h.dtype == torch.float32:
        h = h.view(torch.uint32)
    if tk is not None:  # a time series: the pyramid of the deltas, in the signed dtype of the samples' width
        h = delta.d_encode(h, tk[0])
    x, arrays, meta_levels, levels = _lossless_levels(h, predictor, levels)
    meta = {'format': 'kompressor_amd', 'ndim': ndim, 'padding': padding, 'method': method,
            'sample_dtype': sample, 'levels': meta_levels, 'lowres_shape': list(x.shape),
            'predictor': _predictor_meta(predictor, padding, ndim, x.dtype)}
    if tk is not None:
        meta['temporal'] = _temporal_meta(tk, h)
    # one bundle: the coarsest lowres, then every level's maps finest first (no bundle dims: the
    # per-level dims live in the metadata)
    return {'x': x, 'arrays': arrays, 'meta': meta, 'levels': levels}


def _parts_near(h, predictor, levels, method, max_error):
    """The closed loop of ``max_error > 0``; ``'restored'`` is what the file decodes to."""
    ndim, padding = predictor.ndim, predictor.padding
    levels = _auto_levels(h.shape, ndim) if levels == 'auto' else int(levels)
    _nd._require(levels >= 1, 'levels must be >= 1')
    lowres, encoded, restored = near.d_encode_pyramid(predictor, h, levels, near.coder_id(h.dtype, max_error))
    arrays, meta_levels, shape = [], [], list(h.shape)
    for maps, dims in encoded:
        arrays.extend(maps)
        meta_levels.append({'highres_shape': list(shape), 'dims': [int(d) for d in dims]})
        shape = [shape[0], *[(s + 1) // 2 for s in shape[1:1 + ndim]], *shape[1 + ndim:]]
    meta = {'format': 'kompressor_amd', 'ndim': ndim, 'padding': padding, 'method': method,
            'sample_dtype': _NP_NAME[h.dtype], 'levels': meta_levels, 'lowres_shape': list(lowres.shape),
            'predictor': _predictor_meta(predictor, padding, ndim, h.dtype), 'max_error': max_error}
    return {'x': lowres, 'arrays': arrays, 'meta': meta, 'levels': levels, 'restored': restored}


def _compress_near(path, h, predictor, levels, method, tile_crc, max_error, t0):
    """:func:`compress` with ``max_error > 0``: the closed loop, the bound's check, the version-4 file."""
    p = _parts_near(h, predictor, levels, method, max_error)
    worst = near.d_max_abs_error(p['restored'], h)
    if worst > max_error:
        raise RuntimeError(f'near-lossless encode broke its bound: max |restored - highres| = {worst} > max_error = '
                           f'{max_error}; nothing written to {path}')
    blob, total, crc, table = _bundle(p['x'], p['arrays'], (), method, tile_crc)
    nbytes = _write(path, p['meta'], blob, total, crc, t0, table, VERSION_NEAR)
    raw = h.numel() * h.element_size()
    return {'bytes': nbytes, 'raw_bytes': raw, 'ratio': raw / nbytes, 'bits_per_sample': 8.0 * nbytes / h.numel(),
            'levels': p['levels'], 'max_error': max_error, 'max_abs_error': worst,
            **_quality(metrics.d_compare(h.reshape(-1), p['restored'].reshape(-1)), h.dtype)}


def _restored_record(h, n, dequantise, exceptions):
    """The comparing call (``metrics.d_compare``) of the float32 device tensor ``h`` against exactly what
    :func:`decompress` returns for the quantised ``n``: slab by slab -- ``dequantise(slab of n)``, the slab's
    exceptions put back, the comparison continuing one record -- so the temporaries stay bounded.
    Returns the device record (None for an empty array); nothing is read back but, when there are
    exceptions, the slabs' positions in the index list (once)."""
    hf, nf = h.reshape(-1), n.reshape(-1)
    cuts = [*range(0, hf.numel(), _QUANT_SLAB), hf.numel()]
    if exceptions is not None:
        idx, bits = exceptions
        at = torch.searchsorted(idx, torch.tensor(cuts, device='cuda')).tolist()
    record = None
    for k, (s, e) in enumerate(zip(cuts, cuts[1:])):
        r = dequantise(nf[s:e])
        if exceptions is not None and at[k + 1] > at[k]:
            r.view(torch.int32)[idx[at[k]:at[k + 1]] - s] = bits[at[k]:at[k + 1]].view(torch.int32)
        record = metrics.d_compare(hf[s:e], r, record)
    return record


def _quality(record, dtype, peak=None):
    """``{'mse', 'psnr', 'value_range'}`` of a device record (one read-back; None: nothing compared)."""
    words = metrics.record_words(record) if record is not None else metrics._empty_words()
    q = metrics.summary(words, dtype, peak)
    return {'mse': q['mse'], 'psnr': q['psnr'], 'value_range': q['value_range']}


def _quant_max_error(h, n, exp, exceptions):
    """``max |restore - h|`` over the non-exceptions, in float64, as a Python float: the dequantising
    launch and the difference run slab by slab, so the temporaries stay bounded; one read-back."""
    hf, nf = h.reshape(-1), n.reshape(-1)
    worst = torch.zeros((), dtype=torch.float64, device='cuda')
    idx = None if exceptions is None else exceptions[0]
    for s in range(0, hf.numel(), _QUANT_SLAB):
        e = min(s + _QUANT_SLAB, hf.numel())
        d = (quant.d_code(_lib_decode, n.dtype, exp, nf[s:e]).double() - hf[s:e].double()).abs_()
        if idx is not None:
            i0, i1 = torch.searchsorted(idx, torch.tensor([s, e], device='cuda')).tolist()
            d[idx[i0:i1] - s] = 0.0
        worst = torch.maximum(worst, d.max())
    return float(worst.item())


def _parts_quantised(h, predictor, levels, method, key, param, value, quantise, runs=False, tk=None):
    """The quantiser (``quantise(h, value)``), the lossless pyramid of its integers ``'n'``, the
    exceptions ``'exc'`` (``'E'`` of them) behind the maps, the metadata's ``key`` entry.  ``runs``: the
    integers under the exceptions are hold-filled and the exceptions ride as ``'R'`` runs.  ``tk``: a time
    series -- the pyramid is that of the deltas of ``'n'`` (as the file restores it: after marks and fill)."""
    ndim, padding = predictor.ndim, predictor.padding
    n, exc = quantise(h, value, marks=runs)  # runs: the marks ENCODE wrote stay in n
    E = 0 if exc is None else int(exc[0].numel())
    if E and runs:  # n is this call's own tensor: filled in place (kmp_code allows out == x for the fill)
        n = quant.d_fill(n, out=n)
    x, arrays, meta_levels, levels = _lossless_levels(n if tk is None else delta.d_encode(n, tk[0]), predictor, levels)
    R = 0
    if E and runs:  # the runs ride behind the maps: start gap words (low, high), lengths, bit deltas
        stored = quant.d_runs(*exc)
        arrays, R = [*arrays, *stored], int(stored[0].numel())
    elif E:  # the exceptions ride behind the maps: gap words (low, high), then the bits
        arrays = [*arrays, *quant.d_gaps(exc[0]), exc[1]]
    meta = {'format': 'kompressor_amd', 'ndim': ndim, 'padding': padding, 'method': method,
            'sample_dtype': 'float32', 'levels': meta_levels, 'lowres_shape': list(x.shape),
            'predictor': _predictor_meta(predictor, padding, ndim, x.dtype),
            key: {param: value, 'dtype': _NP_NAME[n.dtype], 'exceptions': E}}
    if R:
        meta['exception_runs'] = R
    if tk is not None:
        meta['temporal'] = _temporal_meta(tk, n)
    return {'x': x, 'arrays': arrays, 'meta': meta, 'levels': levels, 'n': n, 'exc': exc, 'E': E, 'R': R}


def _parts_quant(h, predictor, levels, method, exp, runs=False, tk=None):
    return _parts_quantised(h, predictor, levels, method, 'quant', 'exp', exp, quant.d_quantise, runs, tk)


def _parts_prec(h, predictor, levels, method, bits, runs=False, tk=None):
    return _parts_quantised(h, predictor, levels, method, 'prec', 'bits', bits, quant.d_quantise_rel, runs, tk)


def _compress_quant(path, h, predictor, levels, method, tile_crc, abs_error, exp, t0, runs=False, tk=None):
    """:func:`compress` with ``abs_error``: the quantiser, the lossless pyramid of its integers, the
    bound's check, the version-5 file."""
    p = _parts_quant(h, predictor, levels, method, exp, runs, tk)
    n, E = p['n'], p['E']
    eps = quant.effective(abs_error)
    worst = _quant_max_error(h, n, exp, p['exc'])
    if not worst <= eps:
        raise RuntimeError(f'error-bounded encode broke its bound: max |restored - highres| = {worst} > {eps} '
                           f'(abs_error = {abs_error}); nothing written to {path}')
    blob, total, crc, table = _bundle(p['x'], p['arrays'], (), method, tile_crc)
    nbytes = _write(path, p['meta'], blob, total, crc, t0, table,
                    _versioned(p['meta'], VERSION_RUNS if p['R'] else VERSION_QUANT))
    raw = h.numel() * h.element_size()
    return {'bytes': nbytes, 'raw_bytes': raw, 'ratio': raw / nbytes, 'bits_per_sample': 8.0 * nbytes / h.numel(),
            'levels': p['levels'], 'abs_error': eps, 'abs_error_asked': float(abs_error), 'max_abs_error': worst,
            'exceptions': E, 'quant_dtype': _NP_NAME[n.dtype], **({'exception_runs': p['R']} if runs else {}),
            **_temporal_result(tk),
            **_quality(_restored_record(h, n, lambda s: quant.d_code(_lib_decode, n.dtype, exp, s), p['exc']), h.dtype)}


def _prec_max_error(h, n, bits, exceptions):
    """``max |restore - h| / max(|h|, 2^-126)`` over the non-exceptions, in float64, as a Python float:
    slab by slab like :func:`_quant_max_error`, one read-back."""
    hf, nf = h.reshape(-1), n.reshape(-1)
    worst = torch.zeros((), dtype=torch.float64, device='cuda')
    idx = None if exceptions is None else exceptions[0]
    for s in range(0, hf.numel(), _QUANT_SLAB):
        e = min(s + _QUANT_SLAB, hf.numel())
        xd = hf[s:e].double()
        d = (quant.d_code_rel(_lib_decode, n.dtype, bits, nf[s:e]).double() - xd).abs_() / xd.abs_().clamp_min_(2.0 ** -126)
        if idx is not None:
            i0, i1 = torch.searchsorted(idx, torch.tensor([s, e], device='cuda')).tolist()
            d[idx[i0:i1] - s] = 0.0
        worst = torch.maximum(worst, d.max())
    return float(worst.item())


def _compress_prec(path, h, predictor, levels, method, tile_crc, rel_error, bits, t0, runs=False, tk=None):
    """:func:`compress` with ``rel_error``: the mantissa quantiser, the lossless pyramid of its integers,
    the guarantee's check, the version-6 file."""
    p = _parts_prec(h, predictor, levels, method, bits, runs, tk)
    n, E = p['n'], p['E']
    eps = quant.effective_rel(rel_error)
    worst = _prec_max_error(h, n, bits, p['exc'])
    if not worst <= eps:
        raise RuntimeError(f'relative-error encode broke its bound: max |restored - highres| / max(|highres|, 2^-126) '
                           f'= {worst} > {eps} (rel_error = {rel_error}); nothing written to {path}')
    blob, total, crc, table = _bundle(p['x'], p['arrays'], (), method, tile_crc)
    nbytes = _write(path, p['meta'], blob, total, crc, t0, table,
                    _versioned(p['meta'], VERSION_RUNS if p['R'] else VERSION_PREC))
    raw = h.numel() * h.element_size()
    return {'bytes': nbytes, 'raw_bytes': raw, 'ratio': raw / nbytes, 'bits_per_sample': 8.0 * nbytes / h.numel(),
            'levels': p['levels'], 'rel_error': eps, 'rel_error_asked': float(rel_error), 'max_rel_error': worst,
            'exceptions': E, 'quant_dtype': _NP_NAME[n.dtype], **({'exception_runs': p['R']} if runs else {}),
            **_temporal_result(tk),
            **_quality(_restored_record(h, n, lambda s: quant.d_code_rel(_lib_decode, n.dtype, bits, s), p['exc']),
                       h.dtype)}


def _sized(h, predictor, levels, tile_crc, max_error=0, abs_error=None, rel_error=None, runs=False, tk=None):
    """:func:`compressed_size` of the device tensor ``h`` with checked arguments."""
    if max_error:
        p = _parts_near(h, predictor, levels, 'rice', int(max_error))
        own = {'max_error': int(max_error)}
    elif abs_error is not None:
        p = _parts_quant(h, predictor, levels, 'rice', quant.exponent(abs_error), runs, tk)
        own = {'abs_error': quant.effective(abs_error), 'exceptions': p['E'], 'quant_dtype': _NP_NAME[p['n'].dtype],
               **({'exception_runs': p['R']} if runs else {})}
    elif rel_error is not None:
        p = _parts_prec(h, predictor, levels, 'rice', quant.mantissa_bits(rel_error), runs, tk)
        own = {'rel_error': quant.effective_rel(rel_error), 'exceptions': p['E'], 'quant_dtype': _NP_NAME[p['n'].dtype],
               **({'exception_runs': p['R']} if runs else {})}
    else:
        p = _parts_lossless(h, predictor, levels, 'rice', tk)
        own = {'max_error': 0}
    arrays = [p['x'], *p['arrays']]
    total = packing.bundle_size(arrays)
    tiles = packing._rice_enc_plan(arrays, ())['T'] if tile_crc else None  # the table's entries, as _bundle counts them
    return {'bound_bytes': _bound_bytes(p['meta'], total, tiles), 'bundle_bytes': total,
            'raw_bytes': h.numel() * h.element_size(), 'levels': p['levels'], **own, **_temporal_result(tk)}


def compressed_size(highres, predictor, levels='auto', method='rice', tile_crc=False, max_error=0, abs_error=None,
                    rel_error=None, exceptions='list', temporal=None, key_interval=None):
    """The size of the file :func:`compress` would write for the same arguments, without writing it:
    the same argument checks, the same quantiser and pyramid (or closed loop), then the measuring
    launches of the Rice bundle (``packing.bundle_size``: the arrays are read once, no bundle is
    allocated, 8 bytes come back).  Returns ``{'bound_bytes', 'bundle_bytes', 'raw_bytes', 'levels'}`` and
    the mode's own entries (``'max_error'``; ``'abs_error'`` or ``'rel_error'`` -- the effective bound --
    with ``'exceptions'`` and ``'quant_dtype'``, and ``'exception_runs'`` under ``exceptions='runs'``, the
    keyword of :func:`compress`; ``'temporal'`` and ``'key_interval'`` under ``temporal='delta'``, the keywords
    of :func:`compress`).  ``bundle_bytes`` is exact.  ``bound_bytes`` is the
    file's length with the metadata's ``crc32`` at its widest, 4294967295 (the CRC is stored as a
    decimal and is not known before the bytes exist): the file written is never larger and at most 16
    bytes smaller.  The bound itself is not checked here (:func:`compress` checks it before it writes).
    ``method='planes'`` raises ValueError: only Rice bundles are sized on the device."""
    _check_bounds(highres, max_error, abs_error, rel_error)  # before the device is touched
    runs = _check_exceptions(exceptions, abs_error, rel_error)
    tk = _check_temporal_args(highres, temporal, key_interval, max_error, abs_error, rel_error)
    packing._check_method(method)
    if method != 'rice':
        raise ValueError("compressed_size needs method='rice' (only Rice bundles are sized on the device)")
    h, _ = dev.to_device(highres)
    return _sized(h, predictor, levels, tile_crc, max_error, abs_error, rel_error, runs, _single_frame(tk, h))


def _compress_target(path, h, predictor, levels, tile_crc, mode, target_bits, target_ratio, t0, runs=False, tk=None):
    """:func:`compress` with ``target_bits`` / ``target_ratio``: the ladder of ``mode``, the search over
    it with :func:`compressed_size` as the size of a rung, then the chosen rung written by the
    explicit-bound path (which still checks its bound before it writes)."""
    raw = h.numel() * h.element_size()
    budget = rate.budget_bytes(h.numel(), raw, target_bits, target_ratio)
    if mode == 'abs':
        # the largest finite |x|: one reduction on the device, one read-back
        M = float(torch.where(torch.isfinite(h), h.abs(), torch.zeros((), device=h.device)).max().item()) if h.numel() else 0.0
        ladder = rate.ladder_abs(M)
    elif mode == 'rel':
        ladder = rate.ladder_rel()
    else:
        ladder = rate.ladder_near(h.dtype)

    def size(r):
        key, value = rate.bound_of(mode, ladder[r])
        return _sized(h, predictor, levels, tile_crc, runs=runs, tk=tk, **{key: value})['bound_bytes']
    try:
        r, probes = rate.search(size, len(ladder), budget)
    except rate.Unreachable as e:
        raise ValueError(f'{path}: the target of {budget} bytes cannot be met: the coarsest rung of the {mode!r} '
                         f'ladder has bound_bytes = {e.coarsest}; nothing written') from None
    key, value = rate.bound_of(mode, ladder[r])
    if mode == 'abs':
        out = _compress_quant(path, h, predictor, levels, 'rice', tile_crc, value, ladder[r], t0, runs, tk)
    elif mode == 'rel':
        out = _compress_prec(path, h, predictor, levels, 'rice', tile_crc, value, ladder[r], t0, runs, tk)
    elif value:
        out = _compress_near(path, h, predictor, levels, 'rice', tile_crc, value, t0)
    else:  # rung 0 of the 'near' ladder is the lossless file
        out = _compress_lossless(path, h, predictor, levels, 'rice', tile_crc, t0, tk)
    return dict(out, target_bytes=budget, bound_bytes=dict(probes)[r], probes=[(ladder[q], b) for q, b in probes])


def _self_compare(h):
    """The record of the float32 device tensor ``h`` against itself (one comparing call, one read-back) and the
    largest finite ``|x|``: the value range, the smallest finite value and the 'abs' ladder's ``M``."""
    words = metrics.record_words(metrics.d_compare(h.reshape(-1), h.reshape(-1)))
    return words, (float(np.abs(words.view(np.float64)[4:6]).max()) if words[0] else 0.0)


def _write_rung(path, h, predictor, levels, method, tile_crc, mode, rung, t0, runs, tk):
    """The explicit-bound call that codes ``rung`` of the ladder of ``mode`` (it still checks its bound)."""
    key, value = rate.bound_of(mode, rung)
    if mode == 'abs':
        return _compress_quant(path, h, predictor, levels, method, tile_crc, value, rung, t0, runs, tk)
    if mode == 'rel':
        return _compress_prec(path, h, predictor, levels, method, tile_crc, value, rung, t0, runs, tk)
    if value:
        return _compress_near(path, h, predictor, levels, method, tile_crc, value, t0)
    return _compress_lossless(path, h, predictor, levels, method, tile_crc, t0, tk)  # rung 0 of 'near'


def _compress_psnr(path, h, predictor, levels, method, tile_crc, mode, target, t0, runs=False, tk=None):
    """:func:`compress` with ``target_psnr``: the ladder of ``mode``, ``rate.search_quality`` over it with the
    PSNR of a rung measured on the device -- float32: the quantiser, then restore and compare in slabs;
    integer samples: the closed loop's restored array against the input -- then the chosen rung written
    by the explicit-bound path (which still checks its bound before it writes).  The peak is fixed once."""
    if mode == 'near':
        ladder, peak = rate.ladder_near(h.dtype), float(2 ** (8 * h.element_size()) - 1)
    else:
        # the range of the finite values and the largest finite |x|: one comparing call of h with itself
        words, M = _self_compare(h)
        peak = metrics.summary(words, h.dtype)['value_range']
        ladder = rate.ladder_abs(M) if mode == 'abs' else rate.ladder_rel()

    def psnr(r):
        if mode == 'near':
            if ladder[r] == 0:
                return float('inf')
            restored = _parts_near(h, predictor, levels, method, int(ladder[r]))['restored']
            record = metrics.d_compare(h.reshape(-1), restored.reshape(-1))
        elif mode == 'abs':
            n, exc = quant.d_quantise(h, ladder[r])
            record = _restored_record(h, n, lambda s: quant.d_code(_lib_decode, n.dtype, ladder[r], s), exc)
        else:
            n, exc = quant.d_quantise_rel(h, ladder[r])
            record = _restored_record(h, n, lambda s: quant.d_code_rel(_lib_decode, n.dtype, ladder[r], s), exc)
        return _quality(record, h.dtype, peak if peak > 0 else None)['psnr']
    try:
        r, probes = rate.search_quality(psnr, len(ladder), target)
    except rate.Unreachable as e:
        raise ValueError(f'{path}: target_psnr = {target} dB cannot be met: the finest rung of the {mode!r} ladder '
                         f'reaches {e.finest} dB; nothing written') from None
    out = _write_rung(path, h, predictor, levels, method, tile_crc, mode, ladder[r], t0, runs, tk)
    return dict(out, target_psnr=target, probes=[(ladder[q], v) for q, v in probes])


def _restored_whole(n, dequantise, exceptions):
    """Exactly what :func:`decompress` returns for the quantised ``n``, whole: ``dequantise(n)`` with the
    exceptions put back (one more array of device memory: a window spans slabs, so nothing is cut)."""
    r = dequantise(n.reshape(-1))
    if exceptions is not None:
        idx, bits = exceptions
        r.view(torch.int32)[idx] = bits.view(torch.int32)
    return r.reshape(n.shape)


def _compress_ssim(path, h, predictor, levels, method, tile_crc, mode, target, t0, runs=False, tk=None):
    """:func:`compress` with ``target_ssim``: as :func:`_compress_psnr`, with the mean SSIM of a rung as its
    quality.  Peak, base and the ladder come from the one comparison of ``h`` with itself.  A float32 probe
    is the quantiser, the WHOLE array restored with its exceptions put back (one more array of device memory
    than the PSNR's slabs: a window spans slabs) and one ``metrics.d_ssim`` call; a 'near' probe compares the
    closed loop's restored array, and the lossless rung 0 is 1.0 without a launch."""
    dims = metrics.ssim_dims(h.shape, 'compress(target_ssim=...)')[1:]
    items = metrics._items(h)
    if mode == 'near':
        ladder, peak, base = rate.ladder_near(h.dtype), float(2 ** (8 * h.element_size()) - 1), 0.0
    else:
        words, M = _self_compare(h)
        ladder = rate.ladder_abs(M) if mode == 'abs' else rate.ladder_rel()
        peak, base = metrics._ssim_frame(words, True, None, f'{path}: compress(target_ssim=...)')
    c1, c2 = metrics.ssim_constants(peak)

    def ssim(r):
        if mode == 'near':
            if ladder[r] == 0:
                return 1.0
            restored = _parts_near(h, predictor, levels, method, int(ladder[r]))['restored']
        elif mode == 'abs':
            n, exc = quant.d_quantise(h, ladder[r])
            restored = _restored_whole(n, lambda s: quant.d_code(_lib_decode, n.dtype, ladder[r], s), exc)
        else:
            n, exc = quant.d_quantise_rel(h, ladder[r])
            restored = _restored_whole(n, lambda s: quant.d_code_rel(_lib_decode, n.dtype, ladder[r], s), exc)
        words = metrics.record_words(metrics.d_ssim(items, metrics._items(restored), dims, c1, c2, base))
        return metrics.ssim_summary(words)['ssim']
    try:
        r, probes = rate.search_quality(ssim, len(ladder), target)
    except rate.Unreachable as e:
        raise ValueError(f'{path}: target_ssim = {target} cannot be met: the finest rung of the {mode!r} ladder '
                         f'reaches an SSIM of {e.finest}; nothing written') from None
    out = _write_rung(path, h, predictor, levels, method, tile_crc, mode, ladder[r], t0, runs, tk)
    return dict(out, ssim=dict(probes)[r], target_ssim=target, probes=[(ladder[q], v) for q, v in probes])


def compare(path, highres, peak=None):
    """The quality of the file ``path`` against the array ``highres`` it was made from: :func:`decompress` on
    the device, then ``metrics.compare`` -- ``{'count', 'mismatch', 'max_abs_error', 'mse', 'rmse', 'psnr',
    'nrmse', 'value_range', 'peak'}``.  A shape that is not the file's is ValueError, a dtype that is not
    the file's TypeError, a bad ``peak`` ValueError: all before the device is touched."""
    peak = metrics.check_peak(peak)
    what = info(path)
    dt = near._input_dtype(highres)
    name = _NP_NAME.get(dt) if isinstance(dt, torch.dtype) else np.dtype(dt).name
    if name != what['sample_dtype']:
        raise TypeError(f'{path} holds {what["sample_dtype"]} samples, the array passed {name}')
    if tuple(highres.shape) != tuple(what['shape']):
        raise ValueError(f'{path} holds an array of shape {tuple(what["shape"])}, the array passed has {tuple(highres.shape)}')
    metrics.check_pair(highres, highres, 'container.compare')  # a dtype that is not compared (int32, uint32): TypeError
    return metrics.compare(highres, decompress(path, as_numpy=False), peak)


def ssim(path, highres, peak=None):
    """The structural similarity of the file ``path`` to the array ``highres`` it was made from: :func:`decompress`
    on the device, then ``metrics.ssim`` -- ``{'ssim', 'min_ssim', 'windows', 'skipped', 'peak', 'base'}``.  A shape
    that is not the file's, a rank other than 4 / 5 or a spatial extent below 7 is ValueError, a dtype that is not
    the file's (or has no SSIM) TypeError, a bad ``peak`` ValueError: all before the device is touched."""
    peak = metrics.check_peak(peak)
    what = info(path)
    dt = near._input_dtype(highres)
    name = _NP_NAME.get(dt) if isinstance(dt, torch.dtype) else np.dtype(dt).name
    if name != what['sample_dtype']:
        raise TypeError(f'{path} holds {what["sample_dtype"]} samples, the array passed {name}')
    if tuple(highres.shape) != tuple(what['shape']):
        raise ValueError(f'{path} holds an array of shape {tuple(what["shape"])}, the array passed has {tuple(highres.shape)}')
    metrics.check_pair(highres, highres, 'container.ssim')  # a dtype without an SSIM (int32, uint32): TypeError
    metrics.ssim_dims(highres.shape, 'container.ssim')
    return metrics.ssim(highres, decompress(path, as_numpy=False), peak)


def _quant_exceptions(path, arrays, E, numel):
    """``(indices, bits)`` from a version-5 bundle's last three arrays, checked (E entries each, uint32,
    every index inside the array) before anything is scattered by them."""
    lo, hi, bits = arrays
    if any(a.dtype != torch.uint32 or tuple(a.shape) != (E,) for a in arrays):
        raise ValueError(f'{path}: the exception arrays do not match the metadata ({E} exceptions)')
    idx = quant.d_indices(lo, hi)
    if int(idx.min().item()) < 0 or int(idx.max().item()) >= numel:
        raise ValueError(f'{path}: an exception index lies outside the array (corrupt file)')
    return idx, bits


def _quant_runs(path, arrays, R, numel):
    """The KMP_CODER_RUNS table from a version-7 bundle's last four arrays, checked (R entries each, uint32,
    every run of at least one element and inside the array, the runs ascending and disjoint: one read-back)
    before anything is written by it."""
    if any(a.dtype != torch.uint32 or tuple(a.shape) != (R,) for a in arrays):
        raise ValueError(f'{path}: the exception run arrays do not match the metadata ({R} runs)')
    try:
        return quant.d_run_table(*arrays, numel)
    except ValueError as e:
        raise ValueError(f'{path}: {e} (corrupt file)') from None


def _decode_predictor(path, meta, predictor, dtype):
    """The predictor a file decodes with -- the one passed, or the file's own -- checked against the
    file's padding and a LinearPredictor's arithmetic (``dtype``: the coded samples' torch dtype).
    Shared by :func:`decompress` and :func:`read_region`."""
    pred = predictor or predictor_from_meta(meta)
    if pred is None:
        raise AssertionError(f'{path} was coded with an external predictions_fn '
                             f'({meta["predictor"]["name"] if meta["predictor"] else "unknown"}): pass it')
    padding = meta['padding']
    if isinstance(pred, (MeanPredictor, LinearPredictor)) and pred.padding != padding:
        raise AssertionError(f'{path} was coded with padding {padding}; the predictor passed has {pred.padding}')
    if isinstance(pred, LinearPredictor) and meta['predictor'] and meta['predictor'].get('kind') == 'linear':
        # the two arithmetics are not bit-equal: decoding with the other one returns wrong samples
        _check_arith_rev(meta, path)
        arith = meta['predictor'].get('arith', 'f32')
        if pred.arith == 'auto':  # a default-constructed predictor takes the file's arithmetic
            pred = LinearPredictor(pred.weights, pred.bias, pred.padding, pred.ndim, arith=arith)
        if pred.arith_for(dtype) != arith:
            raise AssertionError(f"{path} was coded with arith='{arith}'; the predictor passed evaluates with "
                                 f"arith='{pred.arith_for(dtype)}'")
    return pred


def decompress(path, predictor=None, as_numpy=True):
    """Decode a file written by :func:`compress` (or :func:`save`) back to the original array, bit
    for bit, coarsest level first.  A file coded with an external predictions_fn needs it passed."""
    t0 = time.perf_counter()
    meta, blob, crc, tm = _read(path)
    _check_crc(path, meta, crc, blob)
    t1 = time.perf_counter()
    lowres, (arrays, bundle_dims) = packing.unpack_encoded(blob)
    q, extra = _quant(meta), None
    if q is not None:
        if lowres.dtype != q[1]:
            raise ValueError(f'{path}: the bundle holds {lowres.dtype} samples, the metadata says {q[1]}')
        if q[2]:  # the three exception arrays behind the maps, or the four run arrays
            k = 4 if _runs(meta) else 3
            if len(arrays) < k:
                raise ValueError(f'{path}: the exception arrays are missing from the bundle')
            arrays, extra = arrays[:-k], arrays[-k:]
    tk = _temporal(meta)
    if tk is not None and lowres.dtype != tk[1]:
        raise ValueError(f'{path}: the bundle holds {lowres.dtype} samples, the metadata says deltas of {tk[1]}')
    pred = _decode_predictor(path, meta, predictor, lowres.dtype)
    ndim, padding = meta['ndim'], meta['padding']
    nmaps = _nd.NMAPS[ndim]
    levels = meta.get('levels') or [{'dims': list(bundle_dims)}]  # save(): one level, dims in the bundle
    if len(arrays) != nmaps * len(levels):
        raise ValueError(f'{path}: {len(arrays)} coded maps for {len(levels)} levels of {nmaps}')
    coder = near.coder_id(lowres.dtype, _max_error(meta))  # the natural lossless coder, or the file's near coder
    dec_fn = _coder_fn(coder, ndim, lowres.dtype)
    x = lowres
    for lvl in reversed(range(len(levels))):
        maps = list(arrays[nmaps * lvl:nmaps * (lvl + 1)])
        dims = tuple(levels[lvl]['dims'])
        if _nd.fused_plan(pred, dec_fn, padding, x.dtype, ndim, 1) is not None:
            out = torch.empty((x.shape[0], *[2 * e - 1 + d for e, d in zip(_nd._sp(x.shape, ndim), dims)],
                               *x.shape[1 + ndim:]), dtype=x.dtype, device='cuda')
            _nd.fused_decode_into(x, maps, dims, pred, coder, out, ndim)
        else:
            out = _nd.decode(pred, dec_fn, x, (maps, dims), padding, ndim)
        x = out
    if tk is not None:  # a time series: the chain of DECODE launches, in place, then the samples' own dtype
        x = delta.d_decode(x, tk[0], out=x)
        if q is None:
            x = x.view(delta.NAMES[meta['sample_dtype']])
    if q is not None and extra is not None and _runs(meta):  # one dequantising launch, then one RUNS launch
        table = _quant_runs(path, extra, _runs(meta), x.numel())
        x = quant.d_patch_runs(q[3](x, q[0], None), table)
    elif q is not None:  # one dequantising launch, then the exceptions' bits
        x = q[3](x, q[0], None if extra is None else _quant_exceptions(path, extra, q[2], x.numel()))
    elif meta.get('sample_dtype') == 'float32':
        x = x.view(torch.float32)
    torch.cuda.current_stream().synchronize()
    t2 = time.perf_counter()
    out = dev.to_host(x) if as_numpy else x
    t3 = time.perf_counter()
    last_timing.clear()
    last_timing.update(read_upload=tm['read_upload'], crc=t1 - tm['t_upload'], device=t2 - t1, d2h=t3 - t2,
                       total=t3 - t0)
    return out


def _coder_fn(coder, ndim, dtype=None):
    from . import utils
    if _nd.is_near(coder):
        return near.coders(dtype, _lib_max_error(coder))[1]
    name = {0: 'decode_values_raw', 1: 'decode_values_uint8', 2: 'decode_values_uint16', 3: 'decode_values_uint32'}
    return getattr(utils, name[coder])


# ---------------------------------------------------------------------------------------------
# partial reads: only the planes / batch items asked for are read, uploaded and decoded
#
# A v2 Rice bundle is tile-addressable (per array a table of u64 word offsets, one per tile of
# 16384 samples, plus per-block side information) and the codec is plane-addressable (output
# planes [z0, z1) of a level need lowres planes slabs.decode_halo(E, z0, z1, p) and that range's
# map planes only).  ``plan_region`` composes the two down the pyramid; ``read_region`` preads
# the table, side-information and payload windows of the touched tiles, decodes them with
# kmp_rice_bundle_decode_ranges into local arrays and runs the fused decode's z-region level by
# level, coarsest first.  The same recurrence runs on every spatial axis (rows=, cols=: the local
# arrays are cropped along z and y, the box is the fused decode's region) and may stop at any
# pyramid level (level=): DESIGN.md §15.
# ---------------------------------------------------------------------------------------------

_TILE = 16384  # samples per tile of a v2 Rice bundle (256 blocks of 64)
# a level whose plane of cells holds at most this many samples is not cropped along rows: a row run
# touches the same tile as its whole plane, so consecutive planes would decode one tile repeatedly
_ROW_CROP_PLANE = _TILE
_CRC_TABLE_WHOLE = 256 << 10  # a per-tile CRC table up to this size is read whole when several ranges need entries


def info(path):
    """What a file holds, from its header and metadata alone (no payload read, no GPU):
    ``{'shape', 'sample_dtype', 'ndim', 'levels', 'padding', 'predictor', 'method', 'version',
    'file_bytes', 'bundle_bytes'}`` -- ``shape`` is the array :func:`decompress` returns, the one a
    :func:`read_region` selection indexes.  A time series also reports ``'temporal'`` (``'delta'``) and
    ``'key_interval'`` (None: frame 0 alone is a key frame)."""
    with open(path, 'rb') as f:
        version, meta, mlen, n = _read_head(f, path)
        size = os.fstat(f.fileno()).st_size
    try:
        shapes = _meta_shapes(meta)
        pred = meta.get('predictor') or {}
        out = {'shape': tuple(shapes[0][0]), 'sample_dtype': meta.get('sample_dtype') or meta.get('lowres_dtype'),
               'ndim': int(meta['ndim']), 'levels': len(shapes), 'padding': int(meta['padding']),
               'predictor': pred.get('kind'), 'method': meta.get('method'), 'version': version,
               'file_bytes': int(size), 'bundle_bytes': int(n)}
        if _max_error(meta):  # only a near-lossless file reports a bound
            out['max_error'] = _max_error(meta)
        if _quant(meta) is not None:  # only an error-bounded or a relative-error file reports its bound
            param, qdt, E, _ = _quant(meta)
            out.update(quant_dtype=_NP_NAME[qdt], exceptions=E, **({'exception_runs': _runs(meta)} if _runs(meta) else {}),
                       **({'rel_error': 2.0 ** -(param + 1)} if 'prec' in meta else {'abs_error': 2.0 ** (param - 1)}))
        if _temporal(meta) is not None:  # only a time series reports its coding along the batch axis
            out.update(temporal='delta', key_interval=_temporal(meta)[0])
        trailer = _tile_crc_trailer(meta, n, size - (_HEAD.size + mlen), path)
        if trailer is not None:  # only a file that has a table reports one
            out['tile_crc'] = trailer[1]
        return out
    except (KeyError, TypeError, IndexError) as e:
        raise ValueError(f'{path}: corrupt metadata ({e!r})') from None


def _meta_tile_counts(meta):
    """The tile count of every bundle array, in bundle order (the coarsest lowres, then each level's
    maps, finest level first), from the metadata's shapes alone."""
    shapes = _meta_shapes(meta)
    return [_tiles(dev.prod(shapes[-1][1]))] + [_tiles(dev.prod(m)) for _, _, maps, _ in shapes for m in maps] + \
        [_tiles(n) for n in _exception_arrays(meta)]


def _exception_arrays(meta):
    """The lengths of the arrays behind the maps: three of E entries in an error-bounded or a
    relative-error file that has exceptions -- four of R entries when they are stored as runs --, none
    in any other file."""
    q = meta.get('quant') or meta.get('prec')
    E = int(q['exceptions']) if isinstance(q, dict) else 0
    R = meta.get('exception_runs')
    if E > 0 and isinstance(R, int) and not isinstance(R, bool) and R > 0:
        return [R] * 4
    return [E] * 3 if E > 0 else []


def _tile_begins(counts):
    """The global table index of every array's first tile: the prefix sum of the tile counts."""
    out, t = [], 0
    for c in counts:
        out.append(t)
        t += c
    return out


def _tile_crc_trailer(meta, bundle_bytes, avail, path='file'):
    """``None`` for a file without a per-tile CRC table, else ``(offset from the bundle's start, T)``
    of its table, checked before anything is sized from it: the table starts at the bundle's end
    padded to 8 bytes, holds one entry per tile of the shapes the metadata records and lies inside the
    ``avail`` bytes the file holds after its metadata."""
    tc = meta.get('tile_crc')
    if tc is None:
        return None
    try:
        off, T = tc['offset'], tc['tiles']
        ok = isinstance(off, int) and isinstance(T, int) and not isinstance(off, bool) and not isinstance(T, bool)
    except (KeyError, TypeError):
        ok = False
    if not ok:
        raise ValueError(f'{path}: corrupt metadata (tile_crc {tc!r})')
    if meta.get('method') != 'rice':
        raise ValueError(f"{path}: a per-tile CRC table in a file whose method is {meta.get('method')!r}")
    if off != int(bundle_bytes) + (-int(bundle_bytes) % 8):
        raise ValueError(f'{path}: the per-tile CRC table is recorded at {off}, the bundle ends at {bundle_bytes}')
    try:
        want = sum(_meta_tile_counts(meta))
    except (KeyError, TypeError, IndexError) as e:
        raise ValueError(f'{path}: corrupt metadata ({e!r})') from None
    if T != want:
        raise ValueError(f'{path}: the per-tile CRC table records {T} tiles, the shapes in the metadata have {want}')
    if off + 4 * T > avail:
        raise ValueError(f'{path}: truncated per-tile CRC table ({off + 4 * T} bytes recorded, {max(avail, 0)} present)')
    return off, T


def _meta_shapes(meta):
    """Per pyramid level, finest first: ``(highres shape, lowres shape, map shapes, dims)`` from the
    metadata alone (a :func:`save` file: one level, the highres shape from the lowres's and dims)."""
    ndim = int(meta['ndim'])
    if meta.get('levels'):
        hs = [tuple(int(s) for s in lv['highres_shape']) for lv in meta['levels']]
    else:
        lo, dims = [int(s) for s in meta['lowres_shape']], [int(d) for d in meta['dims']]
        hs = [(lo[0], *[2 * e - 1 + d for e, d in zip(lo[1:1 + ndim], dims)], *lo[1 + ndim:])]
    out = []
    for h in hs:
        if len(h) < 1 + ndim or any(s < 1 for s in h):
            raise ValueError(f'bad level shape {h} in the metadata')
        lo, maps, dims = _nd.encoded_shapes(h, ndim)
        out.append((tuple(h), tuple(int(s) for s in lo), [tuple(int(s) for s in m) for m in maps], tuple(dims)))
    for (_, lo, _, _), (h, _, _, _) in zip(out, out[1:]):
        if lo != h:
            raise ValueError(f'level shapes in the metadata do not nest ({lo} then {h})')
    if out[-1][1] != tuple(int(s) for s in meta['lowres_shape']):
        raise ValueError('the coarsest lowres shape in the metadata does not match its levels')
    return out


def _clamp_range(r, extent, what):
    if r is None:
        return 0, int(extent)
    lo, hi = max(int(r[0]), 0), min(int(r[1]), int(extent))
    if hi <= lo:
        raise ValueError(f'{what}={tuple(r)} selects nothing of {extent}')
    return lo, hi


def _tiles(n):
    return -(-(-(-n // 64)) // 256) if n > 0 else 0


def _check_level(level, nlev):
    if isinstance(level, bool) or not isinstance(level, (int, np.integer)) or not 0 <= level <= nlev:
        raise ValueError(f'level={level!r}: a file of {nlev} coded levels has levels 0 .. {nlev}')
    return int(level)


def _refuse_image_planes(ndim, planes):
    if planes is not None and ndim != 3:
        raise ValueError('planes selects along the first spatial axis of a volume; an image file takes rows, cols '
                         'and batch')


def _selection(ndim, top, planes, rows, cols):
    """The clamped span of every spatial axis of the level-``k`` array of shape ``top``."""
    _refuse_image_planes(ndim, planes)
    named = (('planes', planes), ('rows', rows), ('cols', cols))[3 - ndim:]
    return [_clamp_range(r, top[1 + a], name) for a, (name, r) in enumerate(named)]


def plan_region(meta, planes=None, batch=None, rows=None, cols=None, level=0):
    """The arrays a selection needs, as a pure function of the file's metadata.  ``level = k`` selects
    pyramid level ``k`` (0: the array ``decompress`` returns; ``L``, the number of coded levels: the
    stored coarsest lowres; level ``k`` is level 0 strided by ``2**k``) and every range is in that
    level's coordinates: ``planes``, ``rows`` and ``cols`` select along z, y and x of a volume,
    ``rows`` and ``cols`` along y and x of an image (``planes`` raises ValueError there),
    ``batch = (b0, b1)`` items of the leading axis.  Ranges are clamped to the array, an empty or
    reversed one raises ValueError, and so does a ``level`` outside ``[0, L]``.

    From level ``k`` down, on every spatial axis, highres span ``[s, e)`` of a level is its output
    span ``(s // 2, (e + 1) // 2)``, which needs the lowres span ``slabs.decode_halo`` of it -- the
    next level's highres span -- and each map's span ``[o0, min(o1, the map's extent))``.  The local
    arrays a level is decoded from are cropped to these spans along the first spatial axis and, for
    volumes, the second; never along the last one (rows are the contiguous unit of the format), whose
    span restricts the codec's region and the final slice only.  From the finest level whose plane of
    cells fits ``_ROW_CROP_PLANE`` samples on, the second axis is not cropped either (a row run would
    touch the plane's one tile anyway).  The even-size ``dims`` apply to a level's local arrays on
    the axes where its local lowres reaches the last node (``at_top``).

    Returns ``{'batch', 'planes', 'rows', 'cols', 'box': the clamped span per spatial axis, 'level',
    'levels': [{'index', 'highres', 'out', 'lowres', 'maps', 'at_top', 'dims' (the first spatial axis,
    as before), 'axes': per spatial axis {'highres', 'out', 'lowres', 'local': the lowres span the
    local arrays hold, 'at_top', 'crop': the span of the level's local output the level above (or the
    selection) keeps}, 'rows', 'cols': the 'axes' entry of that axis, 'at_top_axes'}] from level ``k``
    to the coarsest, 'lowres': the coarsest lowres' span on the first axis, 'lowres_axes': its local
    span per axis, 'arrays': one entry per bundle array in bundle order (the coarsest lowres, then
    every level's maps, finest first) with its full ``shape``, the selected spans ``sel`` (first axis)
    and ``sel_rows``, the ``local_shape`` it is decoded into (None for the maps of levels finer than
    ``k``, which have no ranges), the offsets ``local_at`` and ``local_row_at`` the selection starts at
    there and ``ranges`` [(first sample, end sample, destination sample)] -- one per array, one per
    batch item when only the first axis is restricted, one per batch item and plane (a row run) where
    rows are cropped; an error-bounded file with exceptions has three more entries behind the maps, its
    exception arrays, each read whole --, 'tiles_decoded': tiles the launches decode, counted per range,
    'tiles_total': tiles in the file}``.

    A time series (``'temporal'`` in the metadata) with ``batch = (a, b)`` is planned for the
    frames ``[a - a % K, b)`` -- ``[0, b)`` when only frame 0 is a key frame --, the chain the frames asked for
    are summed along: ``'batch'`` is that range and ``'frames'`` (in such a plan only) the ``(a, b)`` returned."""
    ndim, p = int(meta['ndim']), int(meta['padding'])
    shapes = _meta_shapes(meta)
    nlev = len(shapes)
    nmaps = _nd.NMAPS[ndim]
    _refuse_image_planes(ndim, planes)
    level = _check_level(level, nlev)
    top = shapes[level][0] if level < nlev else shapes[-1][1]
    b0, b1 = asked = _clamp_range(batch, top[0], 'batch')
    tk = _temporal(meta)
    if tk is not None:  # a time series: the chain starts at the key frame at or before the first frame asked for
        b0 -= b0 % tk[0] if tk[0] else b0
    box = _selection(ndim, top, planes, rows, cols)
    bsel = b1 - b0
    ncrop = ndim - 1  # the leading spatial axes local arrays are cropped along

    def entry(shape, sels, local_ext, local_at):
        """``sels``, ``local_ext``, ``local_at``: per cropped axis, the selected span of the array, the
        local array's extent and where the selection starts in it."""
        (s0, s1), z, local_z = sels[0], shape[1], local_ext[0]
        empty = any(e <= s for s, e in sels)
        out = {'shape': tuple(shape), 'sel': (s0, max(s0, s1)), 'local_shape': (bsel, *local_ext, *shape[1 + ncrop:]),
               'local_at': local_at[0], 'sel_rows': (sels[-1][0], max(sels[-1])), 'local_row_at': local_at[-1]}
        if empty:
            out['ranges'] = []
        elif ncrop == 1 or (sels[1] == (0, shape[2]) and local_ext[1] == shape[2]):
            per = dev.prod(shape[2:])
            if (s0, s1) == (0, z) and local_z == z:
                out['ranges'] = [(b0 * z * per, b1 * z * per, 0)]
            else:
                out['ranges'] = [((bi * z + s0) * per, (bi * z + s1) * per, ((bi - b0) * local_z + local_at[0]) * per)
                                 for bi in range(b0, b1)]
        else:  # one row run per batch item and selected plane, compact in the local array
            (r0, r1), y, local_y, per = sels[1], shape[2], local_ext[1], dev.prod(shape[3:])
            out['ranges'] = [(((bi * z + zi) * y + r0) * per, ((bi * z + zi) * y + r1) * per,
                              (((bi - b0) * local_z + local_at[0] + zi - s0) * local_y + local_at[1]) * per)
                             for bi in range(b0, b1) for zi in range(s0, s1)]
        return out

    def small_plane(lo_shape):  # the row-crop threshold: a plane of cells within one tile
        return ndim == 3 and dev.prod(lo_shape[2:]) <= _ROW_CROP_PLANE

    span, target, widened = list(box), list(box), False
    levels, map_entries = [], []
    for j in range(level, nlev):
        h, lo_shape, map_shapes, dims = shapes[j]
        if widened or small_plane(lo_shape):
            widened = True
            span[1] = (0, h[2])
        axes = []
        for a in range(ndim):
            s, e = span[a]
            E = lo_shape[1 + a]
            o0, o1 = s // 2, (e + 1) // 2
            need = (max(0, o0 - 1 - p), min(E, o1 + p + 1))  # slabs.decode_halo
            local = need if a < ncrop else (0, E)
            axes.append({'highres': (s, e), 'out': (o0, o1), 'lowres': need, 'local': local, 'at_top': local[1] == E,
                         'crop': (target[a][0] - 2 * local[0], target[a][1] - 2 * local[0])})
        El = [A['local'][1] - A['local'][0] for A in axes]
        Ll = [el + (dims[a] if axes[a]['at_top'] else 0) for a, el in enumerate(El)]
        msel = []
        for par, ms in zip(_nd.PARITY[ndim], map_shapes):
            sels = [(A['out'][0], min(A['out'][1], ms[1 + a])) for a, A in enumerate(axes[:ncrop])]
            msel.append((sels[0][0], max(sels[0])))
            map_entries.append(entry(ms, sels, [Ll[a] - 1 if par[a] else El[a] for a in range(ncrop)],
                                     [A['out'][0] - A['local'][0] for A in axes[:ncrop]]))
        levels.append({'index': j, 'highres': axes[0]['highres'], 'out': axes[0]['out'], 'lowres': axes[0]['lowres'],
                       'maps': msel, 'at_top': axes[0]['at_top'], 'dims': tuple(dims), 'axes': axes,
                       'rows': axes[ndim - 2], 'cols': axes[ndim - 1],
                       'at_top_axes': tuple(A['at_top'] for A in axes)})
        span = [A['lowres'] for A in axes]
        target = [A['local'] for A in axes]
    lo_shape = shapes[-1][1]
    if level == nlev and small_plane(lo_shape):
        target[1] = (0, lo_shape[2])
    lowres_axes = [target[a] if a < ncrop else (0, lo_shape[1 + a]) for a in range(ndim)]
    skipped = [{'shape': tuple(ms), 'sel': (0, 0), 'local_shape': None, 'local_at': 0, 'sel_rows': (0, 0),
                'local_row_at': 0, 'ranges': []} for _, _, map_shapes, _ in shapes[:level] for ms in map_shapes]
    arrays = [entry(lo_shape, lowres_axes[:ncrop], [e - s for s, e in lowres_axes[:ncrop]], [0] * ncrop)] + \
        skipped + map_entries
    assert len(arrays) == 1 + nmaps * nlev
    # an error-bounded file's exception arrays (gap words, bits; or the four run arrays) are read whole, whatever
    # the selection
    arrays += [{'shape': (E,), 'sel': (0, E), 'local_shape': (E,), 'local_at': 0, 'sel_rows': (0, E), 'local_row_at': 0,
                'ranges': [(0, E, 0)]} for E in _exception_arrays(meta)]
    for i, e in enumerate(arrays):
        e['index'] = i
    return {'batch': (b0, b1), **({} if tk is None else {'frames': asked}),
            'planes': box[0], 'rows': box[ndim - 2], 'cols': box[ndim - 1], 'box': tuple(box),
            'level': level, 'levels': levels, 'lowres': lowres_axes[0], 'lowres_axes': lowres_axes, 'arrays': arrays,
            'tiles_decoded': sum((e - 1) // _TILE - f // _TILE + 1 for ar in arrays for f, e, _ in ar['ranges']),
            'tiles_total': sum(_tiles(dev.prod(ar['shape'])) for ar in arrays)}


def _pread_exact(fd, view, offset, path):
    if dev.pread_into(fd, view, offset) != view.size:
        raise ValueError(f'{path}: truncated ({view.size} bytes at {offset} not present)')


def _region_windows(fd, path, base, nbytes, rplan, plan, crc_table=None):
    """The table, side-information and payload windows of every range of ``plan`` read from the
    bundle at file offset ``base`` into ONE pinned buffer.  Every value read is validated before it
    sizes a read or a launch.  Returns ``(pinned buffer, bytes used, [(array entry, range, offsets in
    the buffer: toff, params, bw, payload, payload_first, payload_words)], payload bytes read, per
    range the buffer offset of its tiles' CRC entries)``.  ``crc_table = (offset of the file's
    per-tile CRC table from the bundle's start, T)`` (validated by the caller) reads the touched
    tiles' u32 entries into the same buffer -- each range's are contiguous -- or the whole table at
    once when that is fewer reads and it is small; without it the last result is empty.

    The ranges of one array and batch item (the row runs of a box selection) share ONE read of the
    tile table and ONE of each side-information array, from their first through their last touched
    tile (8 bytes per tile, 2 per block: the span costs less than a read per run); each range's
    records point into the span.  The payload is one read per range."""
    poff, words = rplan['poff'], rplan['words']
    if rplan['total'] > nbytes:
        raise ValueError(f'{path}: the bundle records {rplan["total"]} bytes, the file holds {nbytes}')
    jobs, groups, used, payload_bytes = [], [], 0, 0
    for ar in plan['arrays']:
        i = ar['index']
        n, code = rplan['ns'][i], rplan['codes'][i]
        W = 8 * torch.empty(0, dtype=dev.CODE_TO_TORCH[code]).element_size()
        side, toff = rplan['offs'][i]
        nb, nt = -(-n // 64), _tiles(n)
        w_first, w_end = rplan['spans'][i]
        per_item = max(dev.prod(ar['shape'][1:]), 1)
        by_item = {}  # the ranges of one batch item (ascending) share one table and one side-information span
        for rng in ar['ranges']:
            by_item.setdefault(rng[0] // per_item, []).append(rng)
        for rngs in by_item.values():
            g0, g1 = rngs[0][0] // _TILE, max((r[1] - 1) // _TILE for r in rngs)
            cnt = g1 - g0 + 1
            have = cnt + 1 if g1 + 1 < nt else cnt  # the table has no entry after the last tile
            tab = np.empty((cnt + 1,), np.uint64)
            _pread_exact(fd, tab[:have].view(np.uint8), base + toff + 8 * g0, path)
            if have == cnt:
                tab[cnt] = w_end
            nside = min(nb, 256 * (g1 + 1)) - 256 * g0
            o_t = used
            o_p = o_t + 8 * (cnt + 1)
            o_b = o_p + nside
            used = (o_b + nside + 7) & ~7
            groups.append((tab, o_t, o_p, o_b, nside, side + 256 * g0, side + ((nb + 7) & ~7) + 256 * g0,
                           len(jobs), len(rngs), g0, cnt))
            for rng in rngs:  # the entries of the tiles a range touches: checked before they size anything
                t0, t1 = rng[0] // _TILE, (rng[1] - 1) // _TILE
                tl = [int(v) for v in tab[t0 - g0:t1 - g0 + 2]]
                if (t0 == 0 and tl[0] != w_first) or tl[0] < w_first or tl[-1] > w_end or w_end > words or \
                        any(y < x or y - x > 256 * (2 * W + 2) for x, y in zip(tl, tl[1:])):
                    raise ValueError(f'{path}: tile table of array {i} is inconsistent (corrupt file)')
                pw = tl[-1] - tl[0]
                if poff + 4 * tl[-1] > nbytes:
                    raise ValueError(f'{path}: payload window of array {i} lies outside the file')
                o_w = used
                used = (o_w + 4 * pw + 7) & ~7
                jobs.append((ar, rng, (o_t + 8 * (t0 - g0), o_p + 256 * (t0 - g0), o_b + 256 * (t0 - g0), o_w, tl[0],
                                       pw)))
                payload_bytes += 4 * pw
    crc_reads, crc_offs = [], []  # (buffer offset, bytes, file offset from the bundle's start)
    if crc_table is not None and jobs:
        c_off, T = crc_table
        begins = _tile_begins([_tiles(n) for n in rplan['ns']])
        if len(jobs) > 1 and 4 * T <= _CRC_TABLE_WHOLE:
            crc_reads.append((used, 4 * T, c_off))
            crc_offs = [used + 4 * (begins[ar['index']] + rng[0] // _TILE) for ar, rng, _ in jobs]
            used = (used + 4 * T + 7) & ~7
        else:  # one read per group: the entries of its first through last touched tile
            for *_, j0, nj, g0, cnt in groups:
                for ar, rng, _ in jobs[j0:j0 + nj]:
                    crc_offs.append(used + 4 * (rng[0] // _TILE - g0))
                crc_reads.append((used, 4 * cnt, c_off + 4 * (begins[jobs[j0][0]['index']] + g0)))
                used = (used + 4 * cnt + 7) & ~7
    buf = dev.pinned_staging(max(used, 8), 'region')
    hv = buf.numpy()
    for tab, o_t, o_p, o_b, nside, f_p, f_b, *_ in groups:
        hv[o_t:o_t + tab.nbytes] = tab.view(np.uint8)
        _pread_exact(fd, hv[o_p:o_p + nside], base + f_p, path)
        _pread_exact(fd, hv[o_b:o_b + nside], base + f_b, path)
    for ar, rng, (_, _, _, o_w, w0, pw) in jobs:
        if pw:
            _pread_exact(fd, hv[o_w:o_w + 4 * pw], base + poff + 4 * w0, path)
    for o, nb_, f_o in crc_reads:
        _pread_exact(fd, hv[o:o + nb_], base + f_o, path)
    return buf, used, jobs, payload_bytes, crc_offs


def _region_restore(meta, plan, x, extra):
    """The float32 box of an error-bounded file from its integer box ``x`` (contiguous): one
    dequantising launch, then the bits of the exceptions that fall in it -- at level ``k`` those whose
    spatial coordinates are all multiples of ``2**k``.  ``extra``: the gap words and the bits, or the four run
    arrays, or None.  Runs are clipped to the flat interval the box spans and only what is left of them is
    expanded to indices.  Every index is masked to the box before it addresses anything, so damaged arrays cannot write
    outside the result (the caller's tile checks report them)."""
    param, _, _, d_restore = _quant(meta)
    out = d_restore(x, param, None)
    if extra is None:
        return out
    ndim, k = int(meta['ndim']), plan['level']
    shape0 = _meta_shapes(meta)[0][0]
    spans = [plan['batch'], *plan['box'], *[(0, s) for s in shape0[1 + ndim:]]]
    if len(extra) == 4:
        # the flat interval of level 0 between the box's first and last element
        first = last = 0
        for a, (s, (lo, hi)) in enumerate(zip(shape0, spans)):
            sh = k if 1 <= a <= ndim else 0
            first, last = first * s + (lo << sh), last * s + min(((hi - 1) << sh), s - 1)
        starts, lengths, rbits = quant.d_run_starts(*extra)
        try:  # inside the array, ascending, disjoint -- as decompress checks them -- before any sum is formed
            quant.d_check_runs(starts, lengths, dev.prod(shape0))
        except ValueError as e:
            raise ValueError(f'{e} (corrupt file)') from None
        ends = torch.clamp(starts + lengths, max=last + 1)
        starts = torch.clamp(starts, min=first)
        inside = ends > starts
        idx, bits = quant.d_expand(starts[inside], (ends - starts)[inside], rbits[inside])
    else:
        idx, bits = quant.d_indices(extra[0], extra[1]), extra[2]
    keep = (idx >= 0) & (idx < dev.prod(shape0))
    flat, rem, stride = torch.zeros_like(idx), idx, 1
    for a in reversed(range(len(shape0))):
        c, rem = rem % shape0[a], rem // shape0[a]
        if 1 <= a <= ndim:
            keep &= (c & ((1 << k) - 1)) == 0
            c = c >> k
        lo, hi = spans[a]
        keep &= (c >= lo) & (c < hi)
        flat += (c - lo) * stride
        stride *= hi - lo
    out.reshape(-1).view(torch.int32)[flat[keep]] = bits.view(torch.int32)[keep]
    return out


def level_shapes(path):
    """The shape of every pyramid level of a file, from its header and metadata alone (no payload
    read, no GPU): ``[level 0 (the array decompress returns), level 1, ..., level L]`` for a file of
    ``L`` coded levels -- level ``L`` is the stored coarsest lowres, level ``k`` is level 0 strided by
    ``2**k`` along every spatial axis, and each is what ``read_region(path, level=k)`` returns."""
    with open(path, 'rb') as f:
        _, meta, _, _ = _read_head(f, path)
    try:
        shapes = _meta_shapes(meta)
    except (KeyError, TypeError, IndexError) as e:
        raise ValueError(f'{path}: corrupt metadata ({e!r})') from None
    return [tuple(h) for h, _, _, _ in shapes] + [tuple(shapes[-1][1])]


def read_region(path, planes=None, batch=None, predictor=None, as_numpy=True, verify=False, tile_crc=True,
                rows=None, cols=None, level=0):
    """``decompress(path)[b0:b1, z0:z1, y0:y1, x0:x1]`` -- bit for bit, contiguous, in the file's
    sample dtype -- reading, uploading and decoding only what the selection needs.
    ``batch=(b0, b1)`` selects items of the leading axis (any file: "tile 37" of a tiled file is
    ``batch=(37, 38)``); ``planes=(z0, z1)``, ``rows=(y0, y1)`` and ``cols=(x0, x1)`` select along z,
    y and x of a volume file, ``rows`` and ``cols`` along y and x of an image file (``planes`` raises
    ValueError there).  ``level=k`` reads pyramid level ``k`` instead (:func:`level_shapes`): the
    result is ``decompress(path)[:, ::2**k, ::2**k, ::2**k][b0:b1, z0:z1, y0:y1, x0:x1]`` and every
    range is in level-``k`` coordinates; the arrays of finer levels are neither read nor decoded, and
    ``level=L`` (the stored coarsest lowres) runs no codec kernel.  Ranges are clamped; an empty one
    raises ValueError, and so does a ``level`` outside ``[0, L]``.  ``predictor`` as for
    :func:`decompress`.  A time series (``temporal='delta'``) reads the same box of the frames from the key
    frame at or before ``b0`` (frame 0 without a ``key_interval``), sums along the chain and returns
    ``b0 .. b1``.

    What a range saves: planes and (for a volume whose planes exceed one tile, ``plan_region``) rows
    crop the arrays read and decoded; a column range does not -- rows are the format's contiguous
    unit, every touched row is read and Rice-decoded whole -- but restricts the codec's region and
    the samples returned.

    Integrity: a partial read cannot check the bundle's CRC-32 and does not.  Every table entry read
    is validated on the host, and the decode checks the side information of every tile it touches
    (a corrupt touched tile raises ValueError).  A file written with ``tile_crc=True`` carries one
    CRC-32 per tile: the entries of the touched tiles are read with the windows, uploaded in the same
    transfer and compared on the device (``kmp_rice_tile_crc`` over the very windows the decode
    reads), their counter returned by the read's one synchronisation -- a damaged touched tile raises
    ValueError (``tile_crc=False`` skips the check; ``last_timing['tile_crc']`` says whether it ran).
    Without a table, damage that keeps a touched tile's side information consistent decodes to wrong
    samples silently.  Corruption in tiles the selection does not touch is not noticed either way.
    ``verify=True`` first reads and CRC-checks the whole bundle, then decodes only the region.

    Files without a v2 Rice bundle ('planes' files, version-1 files) are read by a full
    :func:`decompress` plus a stride and a slice (``last_timing['partial']`` is False).  Host and
    device memory are proportional to the selection (plus its halo at every level, in full rows)."""
    t0 = time.perf_counter()
    if verify:
        vmeta, vblob, vcrc, _ = _read(path)
        _check_crc(path, vmeta, vcrc)
        del vblob
    dev.require_gpu()
    with open(path, 'rb') as f:
        version, meta, mlen, nbytes = _read_head(f, path)
        fd, base = f.fileno(), _HEAD.size + mlen
        hb = os.pread(fd, min(packing._RHEAD.size, nbytes), base)
        partial = version >= 2 and meta.get('method') == 'rice' and hb[:4] == packing.BUNDLE_MAGIC and \
            len(hb) == packing._RHEAD.size and struct.unpack('<H', hb[4:6])[0] == packing.RICE_VERSION
        if not partial:  # no tile table to address: the whole file, then the stride and the slice
            try:
                ndim = int(meta['ndim'])
                level = _check_level(level, len(_meta_shapes(meta)))
            except (KeyError, TypeError, IndexError) as e:
                raise ValueError(f'{path}: corrupt metadata ({e!r})') from None
            _refuse_image_planes(ndim, planes)  # before the decode, not after
            out = decompress(path, predictor, as_numpy)
            if level:
                out = out[(slice(None), *[slice(None, None, 2 ** level)] * ndim)]
            b0, b1 = _clamp_range(batch, out.shape[0], 'batch')
            box = _selection(ndim, out.shape, planes, rows, cols)
            out = out[(slice(b0, b1), *[slice(s, e) for s, e in box])]
            last_timing.update(partial=False, tiles_decoded=0, tiles_total=0, payload_bytes_read=int(nbytes),
                               bundle_bytes=int(nbytes), total=time.perf_counter() - t0, tile_crc=False, level=level)
            return np.ascontiguousarray(out) if as_numpy else out.contiguous()
        try:
            plan = plan_region(meta, planes, batch, rows, cols, level)
        except (KeyError, TypeError, IndexError) as e:
            raise ValueError(f'{path}: corrupt metadata ({e!r})') from None
        # the file's per-tile CRC table, checked against the file's size and the metadata's shapes
        # before anything is sized from it
        trailer = _tile_crc_trailer(meta, nbytes, os.fstat(fd).st_size - base, path) if tile_crc else None
        count = packing._RHEAD.unpack(hb)[2]
        if not 1 <= count <= packing._MAX_ARRAYS:
            raise ValueError(f'{path}: bad rice bundle header (count {count})')
        head = packing._RHEAD.size + packing._RREC.size * count
        if head > nbytes:
            raise ValueError(f'{path}: truncated bundle')
        hb = os.pread(fd, head, base)
        if len(hb) != head:
            raise ValueError(f'{path}: truncated bundle')
        rplan = packing._rice_dec_plan(None, hb)
        arrays = plan['arrays']
        if [tuple(s) for s in rplan['shapes']] != [ar['shape'] for ar in arrays]:
            raise ValueError(f'{path}: the bundle\'s arrays do not match the metadata\'s levels')
        dtype = dev.CODE_TO_TORCH[rplan['codes'][0]]
        q = _quant(meta)
        if q is not None and dtype != q[1]:
            raise ValueError(f'{path}: the bundle holds {dtype} samples, the metadata says {q[1]}')
        tk = _temporal(meta)
        if tk is not None and dtype != tk[1]:
            raise ValueError(f'{path}: the bundle holds {dtype} samples, the metadata says deltas of {tk[1]}')
        nexc = len(_exception_arrays(meta))
        if q is not None and q[2] and any(dev.CODE_TO_TORCH[c] != torch.uint32 for c in rplan['codes'][-nexc:]):
            raise ValueError(f'{path}: the exception arrays of the bundle are not uint32')
        pred = _decode_predictor(path, meta, predictor, dtype)
        buf, used, jobs, payload_bytes, crc_offs = _region_windows(fd, path, base, nbytes, rplan, plan, trailer)
    t1 = time.perf_counter()
    # ---- one upload of all windows, one ranged decode per run of 32 same-dtype records into the
    # local arrays (samples outside the selection stay unwritten: the codec's region never reads
    # them; the maps of levels finer than the one asked for have no local array) ----
    win = dev.empty((max(used, 8),), torch.uint8)
    win[:used].copy_(buf[:used], non_blocking=True)
    local = [dev.empty(ar['local_shape'], dev.CODE_TO_TORCH[rplan['codes'][ar['index']]])
             if ar['local_shape'] is not None else None for ar in arrays]
    wp = win.data_ptr()
    records = []
    for ar, (first, end, dst), (o_t, o_p, o_b, o_w, w0, pw) in jobs:
        i = ar['index']
        t = local[i]
        records.append((rplan['codes'][i], t.data_ptr() + dst * t.element_size(), rplan['ns'][i], first, end,
                        wp + o_p, wp + o_b, wp + o_t, wp + o_w, w0, pw))
    bad = torch.zeros((2,), dtype=torch.int64, device='cuda')  # [inconsistent tiles, tile CRC mismatches]
    tiles = packing._launch_ranges(records, bad) if records else 0
    if crc_offs:  # the touched tiles' CRCs over the same windows, compared with the file's entries on the device
        packing._launch_tile_crc(
            [(rplan['ns'][ar['index']], first // _TILE, (end - 1) // _TILE, wp + o_p, wp + o_b, wp + o_t,
              wp + o_t + 8 * ((end - 1) // _TILE - first // _TILE + 1), wp + o_w, w0, pw, None, wp + o_e)
             for (ar, (first, end, _), (o_t, o_p, o_b, o_w, w0, pw)), o_e in zip(jobs, crc_offs)], bad[1:])
    # ---- the pyramid, coarsest level first down to the level asked for, each level's region (the z
    # slab alone where the cross-section is whole, else the box) on its local arrays ----
    ndim, padding = meta['ndim'], meta['padding']
    nmaps = _nd.NMAPS[ndim]
    coder = near.coder_id(dtype, _max_error(meta))
    dec_fn = _coder_fn(coder, ndim, dtype)
    x = local[0]
    for L in reversed(plan['levels']):
        lvl, ax = L['index'], L['axes']
        maps = local[1 + nmaps * lvl:1 + nmaps * (lvl + 1)]
        ldims = tuple(d if A['at_top'] else 0 for d, A in zip(L['dims'], ax))
        E = _nd._sp(x.shape, ndim)
        region = [(A['out'][0] - A['local'][0], A['out'][1] - A['local'][0]) for A in ax]
        whole = all(r == (0, e) for r, e in zip(region, E))
        if _nd.fused_plan(pred, dec_fn, padding, x.dtype, ndim, 1) is not None:
            out = dev.empty((x.shape[0], *[2 * e - 1 + d for e, d in zip(E, ldims)], *x.shape[1 + ndim:]), x.dtype)
            _nd.fused_decode_into(x, maps, ldims, pred, coder, out, ndim, region=None if whole else region)
        else:
            if not whole:  # an opaque predictions_fn decodes the whole local array: no stray values in it
                for m, ar in zip(maps, arrays[1 + nmaps * lvl:1 + nmaps * (lvl + 1)]):
                    sl = [slice(None), slice(ar['local_at'], ar['local_at'] + ar['sel'][1] - ar['sel'][0])]
                    if ndim == 3:
                        sl.append(slice(ar['local_row_at'], ar['local_row_at'] + ar['sel_rows'][1] - ar['sel_rows'][0]))
                    keep = m[tuple(sl)].clone()
                    m.view(torch.uint8).zero_()
                    m[tuple(sl)] = keep
            out = _nd.decode(pred, dec_fn, x, (maps, ldims), padding, ndim)
        x = out[(slice(None), *[slice(*A['crop']) for A in ax])]
        if lvl > plan['level']:
            x = x.contiguous()
    if not plan['levels']:  # the stored coarsest lowres itself
        x = x[(slice(None), *[slice(s - lo, e - lo) for (s, e), (lo, _) in zip(plan['box'], plan['lowres_axes'])])]
    if tk is not None:  # a time series: the chain from its key frame, in place, then the frames asked for
        x = x.contiguous()
        x = delta.d_decode(x, tk[0], out=x)[plan['frames'][0] - plan['batch'][0]:]
        plan = dict(plan, batch=plan['frames'])
        if q is None:
            x = x.view(delta.NAMES[meta['sample_dtype']])
    if q is not None:
        x = _region_restore(meta, plan, x.contiguous(), local[-nexc:] if q[2] else None)
    elif meta.get('sample_dtype') == 'float32':
        x = x.contiguous().view(torch.float32)
    nbad, ncrc = bad.tolist()  # the synchronisation
    if nbad:
        raise ValueError(f'{path}: side information is inconsistent in {nbad} of the {tiles} tiles read (corrupt file)')
    if ncrc:
        raise ValueError(f'{path}: tile CRC mismatch in {ncrc} of the {tiles} tiles read (corrupt file)')
    t2 = time.perf_counter()
    out = np.ascontiguousarray(dev.to_host(x)) if as_numpy else x.contiguous()
    t3 = time.perf_counter()
    last_timing.clear()
    last_timing.update(read=t1 - t0, device=t2 - t1, d2h=t3 - t2, total=t3 - t0, partial=True,
                       tiles_decoded=int(tiles), tiles_total=int(plan['tiles_total']),
                       payload_bytes_read=int(payload_bytes), bundle_bytes=int(nbytes), tile_crc=bool(crc_offs),
                       level=plan['level'])
    return out
