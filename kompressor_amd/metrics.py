"""Quality metrics of a restored array against its original, on the device -- a build extension with no
reference counterpart.

One ``kmp_code`` call with ``KMP_CODER_COMPARE`` reads both arrays once and leaves a RECORD of eight 64-bit
words on the device (``include/kompressor_hip.h``): the count of compared elements, the mismatches, the
largest ``|r - x|``, the sum of squared errors and the range of the compared originals.  For float32 an
element is compared iff both values are finite, and is a mismatch iff it is not compared and the two
bit patterns differ; every element of uint8 / uint16 / int8 / int16 arrays is compared.  Everything
else -- ``mse``, ``rmse``, ``psnr``, ``nrmse`` -- is host arithmetic on those words (:func:`summary`):

* ``peak`` defaults to the value range of the compared originals for float32 (SZ's convention) and to
  ``2^W - 1`` for integer samples;
* ``psnr = inf`` if ``mse == 0``, else ``-inf`` if ``peak == 0``, else ``10 log10(peak^2 / mse)``;
* ``nrmse = rmse / peak`` (``inf`` when ``peak == 0`` and ``rmse > 0``).

The record is deterministic: the same buffers give the same 64-bit words on every call.
"""

import math

import numpy as np
import torch

from . import _device as dev
from . import _lib
from ._lib import check, lib

DTYPES = (torch.float32, torch.uint8, torch.uint16, torch.int8, torch.int16)
_NAMES = {'float32': torch.float32, 'uint8': torch.uint8, 'uint16': torch.uint16, 'int8': torch.int8,
          'int16': torch.int16}
RECORD_WORDS = 8
_INF_BITS, _NINF_BITS = 0x7ff0000000000000, 0xfff0000000000000 - (1 << 64)  # as int64


def _torch_dtype(dtype):
    if isinstance(dtype, torch.dtype):
        t = dtype
    else:
        try:
            t = _NAMES.get(np.dtype(dtype).name)
        except TypeError:
            t = None
    if t not in DTYPES:
        raise TypeError(f'kompressor_amd.metrics: {dtype!r} samples are not compared (float32, uint8, uint16, int8, '
                        f'int16)')
    return t


def _input_dtype(x):
    return x.dtype if isinstance(x, torch.Tensor) else np.asarray(x).dtype


def check_peak(peak):
    """``peak`` as a float, or None; ValueError unless it is None or a positive finite number."""
    if peak is None:
        return None
    if isinstance(peak, (bool, str, bytes)) or not isinstance(peak, (int, float, np.integer, np.floating)):
        raise ValueError(f'peak must be a positive finite number, got {peak!r}')
    try:
        p = float(peak)
    except OverflowError:
        p = math.inf
    if not math.isfinite(p) or p <= 0:
        raise ValueError(f'peak must be a positive finite number, got {peak!r}')
    return p


def check_pair(original, restored, who='metrics.compare'):
    """The two arrays of a comparison, checked on the host alone: the torch dtype.  TypeError for an
    unsupported dtype or two different ones, ValueError for two shapes."""
    dt, dr = _input_dtype(original), _input_dtype(restored)
    t = _torch_dtype(dt)
    if _torch_dtype(dr) != t:
        raise TypeError(f'{who}: the original holds {dt} samples, the restored array {dr}')
    so = tuple(original.shape) if isinstance(original, torch.Tensor) else np.shape(original)
    sr = tuple(restored.shape) if isinstance(restored, torch.Tensor) else np.shape(restored)
    if tuple(so) != tuple(sr):
        raise ValueError(f'{who}: the original has shape {tuple(so)}, the restored array {tuple(sr)}')
    return t


def d_record():
    """A device buffer of ``COMPARE_BYTES`` (int64 words) holding the record of nothing compared."""
    buf = torch.zeros((_lib.COMPARE_BYTES // 8,), dtype=torch.int64, device='cuda')
    buf[4:6] = torch.tensor([_INF_BITS, _NINF_BITS], dtype=torch.int64)
    return buf


def d_compare(x, r, record=None):
    """One ``kmp_code`` call on two contiguous device tensors of one dtype and size (``x`` the original):
    the device buffer whose first eight 64-bit words are the record.  ``record`` = a buffer this
    function returned: the call continues it, so a large array is walked slab by slab with one
    read-back at the end."""
    if x.dtype != r.dtype or x.numel() != r.numel() or x.dtype not in DTYPES:
        raise TypeError(f'metrics.d_compare: two tensors of one size and of one of {DTYPES}')
    if x.numel() == 0:
        return d_record() if record is None else record
    buf = dev.empty((_lib.COMPARE_BYTES // 8,), torch.int64) if record is None else record
    check(lib.kmp_code(_lib.ENCODE, _lib.coder_compare(record is not None), dev.dtype_code(r), r.data_ptr(),
                       dev.dtype_code(x), x.data_ptr(), x.numel(), buf.data_ptr(), dev.stream()), 'compare')
    return buf


def record_words(buf):
    """The eight uint64 words of the record in a :func:`d_compare` buffer (one read-back)."""
    return buf[:RECORD_WORDS].cpu().numpy().view(np.uint64)


def summary(record_words, dtype, peak=None):
    """The host arithmetic on a record's eight 64-bit words for samples of ``dtype``: ``{'count',
    'mismatch', 'max_abs_error', 'mse', 'rmse', 'psnr', 'nrmse', 'value_range', 'peak'}``."""
    t = _torch_dtype(dtype)
    peak = check_peak(peak)
    w = np.ascontiguousarray(np.asarray(record_words).reshape(-1)[:RECORD_WORDS]).view(np.uint64)
    f = w.view(np.float64)
    count, mismatch, max_abs = int(w[0]), int(w[1]), float(f[2])
    sse = float(f[3]) if t == torch.float32 else int(w[3])
    x_min, x_max = float(f[4]), float(f[5])
    mse = float(sse) / count if count else 0.0
    rmse = math.sqrt(mse)
    value_range = x_max - x_min if count else 0.0
    if peak is None:
        peak = value_range if t == torch.float32 else float(2 ** (8 * t.itemsize) - 1)
    if mse == 0:
        psnr = math.inf
    elif peak == 0:
        psnr = -math.inf
    else:
        psnr = 10.0 * math.log10(peak * peak / mse)
    if peak == 0:
        nrmse = math.inf if rmse > 0 else 0.0
    else:
        nrmse = rmse / peak
    return {'count': count, 'mismatch': mismatch, 'max_abs_error': max_abs, 'mse': mse, 'rmse': rmse, 'psnr': psnr,
            'nrmse': nrmse, 'value_range': value_range, 'peak': peak}


def _empty_words():
    return np.array([0, 0, 0, 0, _INF_BITS, _NINF_BITS + (1 << 64), 0, 0], np.uint64)


def compare(original, restored, peak=None):
    """``{'count', 'mismatch', 'max_abs_error', 'mse', 'rmse', 'psnr', 'nrmse', 'value_range', 'peak'}`` of
    ``restored`` against ``original``: two numpy arrays or CUDA tensors of one shape and one dtype
    (float32, uint8, uint16, int8, int16).  TypeError for an unsupported dtype or two different ones,
    ValueError for two shapes or a ``peak`` that is no positive finite number -- all before the device
    is touched; an empty input is answered on the host."""
    t = check_pair(original, restored)
    peak = check_peak(peak)
    n = original.numel() if isinstance(original, torch.Tensor) else int(np.size(original))
    if n == 0:
        return summary(_empty_words(), t, peak)
    x, _ = dev.to_device(original)
    r, _ = dev.to_device(restored)
    return summary(record_words(d_compare(x, r)), t, peak)
