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

Structural similarity: one ``kmp_code`` call with ``KMP_CODER_SSIM`` leaves the count, the sum
and the minimum of the SSIM index over every 7 x 7 (images) or 7 x 7 x 7 (volumes) window that lies inside one
item (:func:`ssim`, :func:`d_ssim`, :func:`ssim_summary`).
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


# ---- structural similarity ----

SSIM_WINDOW = 7


def ssim_dims(shape, who='metrics.ssim'):
    """``(N, D, H, W)`` of an array of ``shape`` in the package's layouts ``(B, H, W, C)`` / ``(B, D, H, W, C)``
    -- ``N = B * C`` items, ``D = 1`` for images.  ValueError for another rank or a spatial extent below 7."""
    shape = tuple(int(s) for s in shape)
    if len(shape) not in (4, 5):
        raise ValueError(f'{who}: arrays are (B, H, W, C) or (B, D, H, W, C), got shape {shape}')
    spatial = shape[1:-1]
    if min(spatial) < SSIM_WINDOW:
        raise ValueError(f'{who}: every spatial extent must be at least {SSIM_WINDOW} (the window), got {spatial}')
    return (shape[0] * shape[-1], 1 if len(spatial) == 2 else spatial[0], spatial[-2], spatial[-1])


def ssim_constants(peak):
    """``(C1, C2) = ((0.01 L)^2, (0.03 L)^2)`` for the peak ``L``."""
    return (0.01 * peak) ** 2, (0.03 * peak) ** 2


def _items(t):
    """The device tensor ``t`` in one of the package's layouts as contiguous items: channels first."""
    return t if t.shape[-1] == 1 else t.movedim(-1, 1).contiguous()


def d_ssim(x, r, dims, c1, c2, base):
    """One ``kmp_code`` call with ``KMP_CODER_SSIM`` on two contiguous device tensors of one dtype and size
    (``x`` the original) holding items of ``dims = (D, H, W)`` samples each: the device buffer of ``SSIM_BYTES``
    whose first eight 64-bit words are the record."""
    if x.dtype != r.dtype or x.numel() != r.numel() or x.dtype not in DTYPES:
        raise TypeError(f'metrics.d_ssim: two tensors of one size and of one of {DTYPES}')
    D, H, W = (int(d) for d in dims)
    request = np.zeros(8, np.int64)
    request[:3] = (D, H, W)
    request[3:6] = np.array([c1, c2, base], np.float64).view(np.int64)
    buf = dev.empty((_lib.SSIM_BYTES // 8,), torch.int64)
    head = np.zeros(16, np.int64)
    head[3] = _INF_BITS  # the record of nothing counted, for an empty input
    head[8:] = request
    buf[:16] = torch.from_numpy(head).to('cuda')
    check(lib.kmp_code(_lib.ENCODE, _lib.CODER_SSIM, dev.dtype_code(r), r.data_ptr(), dev.dtype_code(x), x.data_ptr(),
                       x.numel(), buf.data_ptr(), dev.stream()), 'ssim')
    return buf


def ssim_summary(words):
    """The host arithmetic on an SSIM record's eight 64-bit words: ``{'ssim', 'min_ssim', 'windows', 'skipped'}``
    -- ``ssim`` the mean over the counted windows, ``nan`` when there are none.  ValueError for a record
    whose status says the request was malformed."""
    w = np.ascontiguousarray(np.asarray(words).reshape(-1)[:RECORD_WORDS]).view(np.uint64)
    f = w.view(np.float64)
    if int(w[4]) != 0:
        raise ValueError(f'metrics.ssim_summary: the kernel refused the request (status {int(w[4])})')
    windows = int(w[0])
    return {'ssim': float(f[2]) / windows if windows else math.nan, 'min_ssim': float(f[3]), 'windows': windows,
            'skipped': int(w[1])}


def _ssim_frame(words, is_float, peak, who):
    """``(peak, base)`` of a comparison from the record of the original against itself (``words``; None for
    integer samples, whose peak is ``2^W - 1`` -- passed in -- and whose base is 0)."""
    if not is_float:
        return peak, 0.0
    f = words.view(np.float64)
    count = int(words[0])
    base = float(f[4]) if count else 0.0
    if peak is None:
        peak = float(f[5]) - float(f[4]) if count else 0.0
        if peak == 0:
            raise ValueError(f'{who}: the finite originals span no range, so there is no default peak and no SSIM')
    return peak, base


def ssim(original, restored, peak=None):
    """``{'ssim', 'min_ssim', 'windows', 'skipped', 'peak', 'base'}`` of ``restored`` against ``original``: the
    mean and the minimum of the structural similarity index over every 7 x 7 (``(B, H, W, C)`` arrays) or
    7 x 7 x 7 (``(B, D, H, W, C)``) window that lies inside one item, uniform weights, sample variances
    (DESIGN.md §23).  Two numpy arrays or CUDA tensors of one shape and dtype (float32, uint8, uint16, int8,
    int16); ``C > 1`` channels are ``C`` times the items, through a channel-first copy.  ``peak`` defaults to
    the range of the finite originals (float32) or ``2^W - 1``; float32 samples enter as ``v - base``, ``base``
    the smallest finite original, and a window holding a non-finite value on either side is ``skipped``.
    TypeError for an unsupported dtype or two different ones, ValueError for two shapes, a rank other than
    4 / 5, a spatial extent below 7 or a bad ``peak`` -- all before the device is touched; a float32 original
    without a value range and no ``peak`` is ValueError after the one comparison with itself."""
    t = check_pair(original, restored, 'metrics.ssim')
    shape = tuple(original.shape) if isinstance(original, torch.Tensor) else np.shape(original)
    _, D, H, W = ssim_dims(shape)
    peak = check_peak(peak)
    x, _ = dev.to_device(original)
    r, _ = dev.to_device(restored)
    return _ssim_of(_items(x), _items(r), (D, H, W), t, peak, 'metrics.ssim')


def _ssim_of(x, r, dims, t, peak, who):
    """:func:`ssim` on contiguous device items with checked arguments."""
    is_float = t == torch.float32
    if not is_float and peak is None:
        peak = float(2 ** (8 * t.itemsize) - 1)
    words = None
    if is_float:
        words = record_words(d_compare(x.reshape(-1), x.reshape(-1)))
    peak, base = _ssim_frame(words, is_float, peak, who)
    c1, c2 = ssim_constants(peak)
    out = ssim_summary(record_words(d_ssim(x, r, dims, c1, c2, base)))
    return dict(out, peak=peak, base=base)


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
