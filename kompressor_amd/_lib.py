"""ctypes binding of ``libkompressor_hip.so`` (the C-ABI in ``include/kompressor_hip.h``).

The shared library is built in-tree by ``kompressor_amd._build`` (``__graft_entry__.build()``).
Importing this module never falls back to anything: a missing library raises ``ImportError``
and a missing / non-gfx950 GPU raises ``RuntimeError`` at the first compute call.
"""

import ctypes
import os

import numpy as np
# torch must be imported BEFORE the CDLL below: torch ships its own libamdhip64.so (SONAME
# libamdhip64.so.7); loaded first, our library's NEEDED libamdhip64.so.7 binds to that same
# runtime, so torch's allocations, streams and events and our launches share ONE HIP runtime.
# Loaded the other way round the process would carry two runtimes and the second to initialise
# sees no GPU.
import torch  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
# KMP_DEBUG=1 loads the variant with device bounds checks (kompressor_amd/_build.py --debug)
_DEFAULT_LIB = 'libkompressor_hip_debug.so' if os.environ.get('KMP_DEBUG', '0') != '0' else 'libkompressor_hip.so'
LIB_PATH = os.environ.get('KOMPRESSOR_HIP_LIB', os.path.join(HERE, _DEFAULT_LIB))

if not os.path.exists(LIB_PATH):
    raise ImportError(f'kompressor_amd: {LIB_PATH} is missing -- build it with '
                      f'`python -m kompressor_amd._build` (hipcc --offload-arch=gfx950)')

lib = ctypes.CDLL(LIB_PATH)

# enums (include/kompressor_hip.h)
KMP_OK, KMP_ERR_ARG, KMP_ERR_UNSUPPORTED, KMP_ERR_LAUNCH = 0, -1, -2, -3
U8, U16, I32, F32, U32, I8, I16 = 0, 1, 2, 3, 4, 5, 6
CODER_RAW, CODER_U8, CODER_U16, CODER_U32 = 0, 1, 2, 3
CODER_NEAR_U8, CODER_NEAR_U16 = 4, 5  # near-lossless: the ``coder`` argument carries coder_near(code, max_error)


def coder_near(code, max_error):
    """KMP_CODER_NEAR(code, max_error): the value an ``int32_t coder`` argument carries."""
    return int(code) | (int(max_error) << 8)


# error-bounded float32 quantisers (kmp_code alone): the argument carries coder_quant(code, exponent)
CODER_QUANT_I16, CODER_QUANT_I32 = 6, 7


def coder_quant(code, exp):
    """KMP_CODER_QUANT(code, exp): the quantiser ``code`` with the step ``2**exp``."""
    return int(code) | ((int(exp) + 127) << 8)


# relative-error float32 quantisers (kmp_code alone): the argument carries coder_prec(code, mantissa bits)
CODER_PREC_I16, CODER_PREC_I32 = 8, 9


def coder_prec(code, m):
    """KMP_CODER_PREC(code, m): the quantiser ``code`` keeping the top ``m`` mantissa bits."""
    return int(code) | ((int(m) + 1) << 8)


# error statistics of a restored array against its original (kmp_code alone, ENCODE alone): the argument
# carries coder_compare(continue); ``out`` is COMPARE_BYTES -- the record, then COMPARE_GROUPS partial records
CODER_COMPARE = 10
COMPARE_GROUPS = 1024
COMPARE_BYTES = 64 * (1 + COMPARE_GROUPS)


def coder_compare(cont=False):
    """KMP_CODER_COMPARE_MODE(cont): start a record (False) or continue the one already in ``out``."""
    return CODER_COMPARE | (int(bool(cont)) << 8)


# masked float32 fields (kmp_code alone).  CODER_FILL (ENCODE alone): the hold-fill of a marked
# int16 / int32 array, ``pred`` the FILL_BYTES of scratch; workgroup g owns the elements from g * fill_span(n).
# CODER_RUNS (DECODE alone): a float32 array patched from a table of (start low, start high, length, bits)
# records, long runs cut into pieces of RUNS_PIECE when the table is built
CODER_FILL, CODER_RUNS = 11, 12
FILL_TILE = 2048
FILL_GROUPS = 1024
FILL_BYTES = 16 * FILL_GROUPS
RUNS_PIECE = 256


def fill_span(n):
    """The elements one workgroup of the fill owns in an array of ``n``: a function of ``n`` alone."""
    tiles = -(-int(n) // FILL_TILE)
    return -(-tiles // FILL_GROUPS) * FILL_TILE


# time series (kmp_code alone): out = x - pred (ENCODE) or x + pred (DECODE) modulo 2^W of two
# arrays of one integer dtype (U8, I8, U16, I16, I32); ``out`` may be ``x``
CODER_DELTA = 13

# structural similarity of a restored array against its original (kmp_code alone, ENCODE alone):
# ``out`` is SSIM_BYTES -- the record, the request (D, H, W, C1, C2, base) the caller writes, then SSIM_GROUPS
# partial records; a workgroup owns SSIM_TILE_H x SSIM_TILE_W window origins over SSIM_TILE_D origins along D
CODER_SSIM = 14
SSIM_GROUPS = 1024
SSIM_BYTES = 64 * (2 + SSIM_GROUPS)
SSIM_TILE_D, SSIM_TILE_H, SSIM_TILE_W = 32, 16, 16


def ssim_groups(n):
    """The workgroups that run for ``n`` samples (each leaves a partial record): a function of ``n`` alone."""
    return min(SSIM_GROUPS, -(-int(n) // (SSIM_TILE_H * SSIM_TILE_W)))


def coder_code(coder):
    return int(coder) & 0xff


def coder_max_error(coder):
    return int(coder) >> 8

ENCODE, DECODE = 0, 1
PRED_MEAN, PRED_LINEAR, PRED_LINEAR_MFMA = 0, 1, 2

_vp = ctypes.c_void_p
_i32 = ctypes.c_int32
_i64 = ctypes.c_int64
_i64p = ctypes.POINTER(ctypes.c_int64)
_i32p = ctypes.POINTER(ctypes.c_int32)
_vpp = ctypes.POINTER(ctypes.c_void_p)
_fp = ctypes.POINTER(ctypes.c_float)


class Predictor(ctypes.Structure):
    _fields_ = [('kind', ctypes.c_int32), ('padding', ctypes.c_int32),
                ('weights', ctypes.c_void_p), ('bias', ctypes.c_void_p)]


class RiceArray(ctypes.Structure):  # kmp_rice_array (include/kompressor_hip.h)
    _fields_ = [('samples', ctypes.c_void_p), ('n', ctypes.c_int64), ('side_off', ctypes.c_int64),
                ('toff_off', ctypes.c_int64), ('rec_off', ctypes.c_int64)]


class RiceRange(ctypes.Structure):  # kmp_rice_range (include/kompressor_hip.h)
    _fields_ = [('samples', ctypes.c_void_p), ('n', ctypes.c_int64), ('first', ctypes.c_int64),
                ('end', ctypes.c_int64), ('params', ctypes.c_void_p), ('bw', ctypes.c_void_p),
                ('toff', ctypes.c_void_p), ('payload', ctypes.c_void_p), ('payload_first', ctypes.c_uint64),
                ('payload_words', ctypes.c_uint64)]


class RiceCrcRange(ctypes.Structure):  # kmp_rice_crc_range (include/kompressor_hip.h)
    _fields_ = [('n', ctypes.c_int64), ('t0', ctypes.c_int64), ('t1', ctypes.c_int64), ('params', ctypes.c_void_p),
                ('bw', ctypes.c_void_p), ('toff', ctypes.c_void_p), ('closing', ctypes.c_void_p),
                ('payload', ctypes.c_void_p), ('payload_first', ctypes.c_uint64), ('payload_words', ctypes.c_uint64),
                ('crc_out', ctypes.c_void_p), ('expect', ctypes.c_void_p)]


class Region(ctypes.Structure):
    _fields_ = [('begin', ctypes.c_int64 * 3), ('end', ctypes.c_int64 * 3)]


_PROTOS = {
    'kmp_version': (ctypes.c_char_p, []),
    'kmp_last_error': (ctypes.c_char_p, []),
    'kmp_last_launch': (ctypes.c_char_p, []),
    'kmp_device_ok': (ctypes.c_int, []),
    'kmp_set_option': (ctypes.c_int, [ctypes.c_char_p, ctypes.c_int]),
    'kmp_clear_option': (ctypes.c_int, [ctypes.c_char_p]),
    'kmp_get_option': (ctypes.c_int, [ctypes.c_char_p, ctypes.POINTER(ctypes.c_int)]),
    'kmp_host_device_pointer': (ctypes.c_int, [_vp, _vpp]),
    'kmp_volume_encode': (ctypes.c_int, [_i32, _vp, _i64, _i64, _i64, _i64, _i64, ctypes.POINTER(Predictor), _i32,
                                         _vp, _vpp, _i32p, ctypes.POINTER(Region), _vp, ctypes.c_size_t, _vp]),
    'kmp_volume_decode': (ctypes.c_int, [_i32, _vp, _vpp, _i64, _i64, _i64, _i64, _i64, _i32p,
                                         ctypes.POINTER(Predictor), _i32, _vp, ctypes.POINTER(Region), _vp,
                                         ctypes.c_size_t, _vp]),
    'kmp_volume_workspace_bytes': (ctypes.c_int64, [_i32, _i64, _i64, _i64, _i64, _i64, ctypes.POINTER(Predictor)]),
    'kmp_image_encode': (ctypes.c_int, [_i32, _vp, _i64, _i64, _i64, _i64, ctypes.POINTER(Predictor), _i32,
                                        _vp, _vpp, _i32p, ctypes.POINTER(Region), _vp, ctypes.c_size_t, _vp]),
    'kmp_image_decode': (ctypes.c_int, [_i32, _vp, _vpp, _i64, _i64, _i64, _i64, _i32p,
                                        ctypes.POINTER(Predictor), _i32, _vp, ctypes.POINTER(Region), _vp,
                                        ctypes.c_size_t, _vp]),
    'kmp_image_workspace_bytes': (ctypes.c_int64, [_i32, _i64, _i64, _i64, _i64, ctypes.POINTER(Predictor)]),
    'kmp_lowres_from_highres': (ctypes.c_int, [_i32, _i32, _vp, _i64, _i64p, _i64, _vp, _vp]),
    'kmp_maps_from_highres': (ctypes.c_int, [_i32, _i32, _vp, _i64, _i64p, _i64, _vpp, _vp]),
    'kmp_targets_from_highres': (ctypes.c_int, [_i32, _i32, _vp, _i64, _i64p, _i64, _vp, _vp]),
    'kmp_highres_from_lowres_and_maps': (ctypes.c_int, [_i32, _i32, _vp, _vpp, _i64, _i64p, _i64, _vp, _vp]),
    'kmp_features_from_lowres': (ctypes.c_int, [_i32, _i32, _vp, _i64, _i64p, _i64, _i32, _vp, _vp]),
    'kmp_maps_from_predictions': (ctypes.c_int, [_i32, _i32, _vp, _i64, _i64p, _i64, _vpp, _vp]),
    'kmp_mean_predict_maps': (ctypes.c_int, [_i32, _i32, _vp, _i64, _i64p, _i64, _i32, _vpp, _vp]),
    'kmp_mean_predict_maps_typed': (ctypes.c_int, [_i32, _i32, _i32, _vp, _i64, _i64p, _i64, _i32, _vpp, _vp]),
    'kmp_linear_predict': (ctypes.c_int, [_i32, _i32, _vp, _i64, _i64p, _i64, _i32, _vp, _vp, _vp, _vp, _vp]),
    'kmp_linear_predict_mfma': (ctypes.c_int, [_i32, _i32, _vp, _i64, _i64p, _i64, _i32, _vp, _vp, _vp, _vp, _vp]),
    'kmp_linear_moments_workspace_bytes': (ctypes.c_size_t, [_i32, _i32, _i32]),
    'kmp_linear_moments': (ctypes.c_int, [_i32, _i32, _vp, _i64, _i64p, _i64, _i32, _vp, _vp, _vp]),
    'kmp_pad': (ctypes.c_int, [_i32, _i32, _vp, _i64, _i64p, _i64, _i64p, _i64p, _i32, _vp, _vp]),
    'kmp_copy_box': (ctypes.c_int, [_i32, _i32, _vp, _i64p, _i64p, _i32, _vp, _i64p, _i64p, _i64, _i64, _i64p,
                                    _vp]),
    'kmp_code': (ctypes.c_int, [_i32, _i32, _i32, _vp, _i32, _vp, _i64, _vp, _vp]),
    'kmp_categorical': (ctypes.c_int, [_i32, _vp, _i64, _i64, _i32, _vp, _vp, _vp]),
    'kmp_tiles': (ctypes.c_int, [_i32, _i32, _i32, _vp, _i64p, _i64, _i64p, _vp, _vp]),
    'kmp_window_from_highres': (ctypes.c_int, [_i32, _i32, _vp, _i64, _i64p, _i64, _i32, _vp, _vp]),
    'kmp_window_from_lowres': (ctypes.c_int, [_i32, _i32, _vp, _i64, _i64p, _i64, _i32p, _i32, _vp, _vp]),
    'kmp_encode_with_predictions': (ctypes.c_int, [_i32, _i32, _i32, _vp, _i64, _i64p, _i64, _vpp, _vp, _vpp,
                                                   _vp]),
    'kmp_pack_blocks': (ctypes.c_int64, [_i64]),
    'kmp_pack_workspace_bytes': (ctypes.c_int64, [_i64]),
    'kmp_pack_total_offset': (ctypes.c_int64, [_i64]),
    'kmp_pack_plan': (ctypes.c_int, [_i32, _vp, _i64, _vp, _vp, _vp]),
    'kmp_pack': (ctypes.c_int, [_i32, _vp, _i64, _vp, _vp, _vp, _vp]),
    'kmp_pack_header': (ctypes.c_int, [_vp, ctypes.c_char_p, _i32, _i64, _i64, _vp, _i64, _i64, _vp]),
    'kmp_unpack_plan': (ctypes.c_int, [_vp, _i64, _vp, _vp]),
    'kmp_unpack': (ctypes.c_int, [_i32, _vp, _i64, _vp, _vp, _vp, _vp]),
    'kmp_unpack_check': (ctypes.c_int, [_i32, _i32, _vp, _vp, _i64, _vp, _vp]),
    'kmp_rice_tiles': (ctypes.c_int64, [_i64]),
    'kmp_rice_bundle_workspace_bytes': (ctypes.c_int64, [_i64]),
    'kmp_rice_bundle_encode': (ctypes.c_int, [_i32, _vp, _i32, _i64, _i64, _vp, _i64, _vp, _vp]),
    'kmp_rice_bundle_decode': (ctypes.c_int, [_i32, _vp, _i32, _i64, _vp, _i64, ctypes.c_uint64, _vp, _vp]),
    'kmp_rice_bundle_decode_ranges': (ctypes.c_int, [_i32, _vp, _i32, _vp, _vp]),
    'kmp_crc32': (ctypes.c_int, [_vp, _i64, _vp, _vp, _vp]),
    'kmp_rice_tile_crc': (ctypes.c_int, [_vp, _i32, _vp, _vp]),
    'kmp_decode_with_predictions': (ctypes.c_int, [_i32, _i32, _i32, _vp, _vpp, _i64, _i64p, _i64, _i32p, _vpp,
                                                   _vp, _vp]),
    'kmp_encode_with_predictions_typed': (ctypes.c_int, [_i32, _i32, _i32, _i32, _vp, _i64, _i64p, _i64, _vpp, _vp,
                                                         _vpp, _vp]),
    'kmp_decode_with_predictions_typed': (ctypes.c_int, [_i32, _i32, _i32, _i32, _vp, _vpp, _i64, _i64p, _i64,
                                                         _i32p, _vpp, _vp, _vp]),
}

for _name, (_res, _args) in _PROTOS.items():
    _fn = getattr(lib, _name)  # AttributeError here == the library does not export the C-ABI
    _fn.restype = _res
    _fn.argtypes = _args

EXPORTED = tuple(_PROTOS)


class KompressorHipError(RuntimeError):
    pass


def check(status, what):
    if status != KMP_OK:
        msg = lib.kmp_last_error().decode(errors='replace')
        raise KompressorHipError(f'{what} failed ({status}): {msg}')


def version():
    return lib.kmp_version().decode()


def get_option(name):
    """A dispatch option's value, or None while it is unset."""
    v = ctypes.c_int()
    r = lib.kmp_get_option(name.encode(), ctypes.byref(v))
    if r < 0:
        check(r, 'kmp_get_option')
    return v.value if r == 1 else None


def set_option(name, value):
    """Set a dispatch option (``None`` returns it to the kernel's own default)."""
    if value is None:
        check(lib.kmp_clear_option(name.encode()), 'kmp_clear_option')
    else:
        check(lib.kmp_set_option(name.encode(), int(value)), 'kmp_set_option')


class option:
    """``with option('KMP_DISABLE_FAST', 1): ...`` -- set a dispatch option for a block, restoring
    its previous state after (the library reads its environment variable only once, at load)."""

    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.prev = get_option(self.name)
        set_option(self.name, self.value)
        return self

    def __exit__(self, *exc):
        set_option(self.name, self.prev)
        return False


# ---------------------------------------------------------------------------------------------
# small ctypes helpers
# ---------------------------------------------------------------------------------------------

def i64x3(vals):
    vals = list(vals) + [0] * (3 - len(vals))
    return (ctypes.c_int64 * 3)(*vals)


def i32xn(vals):
    vals = list(vals)
    return (ctypes.c_int32 * max(3, len(vals)))(*(vals + [0] * (3 - len(vals))))


def ptrs(tensors, n=7):
    arr = (ctypes.c_void_p * n)()
    for i, t in enumerate(tensors):
        arr[i] = t.data_ptr() if t is not None else None
    return arr


_NP_TO_CODE = {np.dtype(np.uint8): U8, np.dtype(np.uint16): U16, np.dtype(np.int32): I32,
               np.dtype(np.float32): F32, np.dtype(np.uint32): U32, np.dtype(np.int8): I8, np.dtype(np.int16): I16}
