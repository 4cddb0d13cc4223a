"""Time series: delta coding along the batch axis -- a build extension with no reference counterpart
(DESIGN.md §22).

``n`` is an integer array of shape ``(T, ...)``, W its width in bits (8, 16 or 32), and the batch axis is
time.  ``key_interval = K``: ``None`` means only frame 0 is a key frame, else ``K >= 1`` and frame ``t`` is a
key frame iff ``t % K == 0``::

    d[t] = n[t]                          key frame
    d[t] = (n[t] - n[t-1]) mod 2**W      otherwise

    n[t] = d[t]                          key frame
    n[t] = (d[t] + n[t-1]) mod 2**W      otherwise

``d`` is stored as the SIGNED type of width W (int8 for uint8 / int8, int16 for uint16 / int16, int32 for
int32; a key frame of unsigned samples is reinterpreted bit for bit), so a small negative difference is a
small signed value.  The delta is exactly invertible whatever the data.  Subsampling commutes with it, so
level ``k`` of a pyramid of ``d`` is the delta of level ``k`` of ``n``.

The arithmetic is ``kmp_code`` with ``KMP_CODER_DELTA``: the encode is one launch over the frames 1 .. T-1
(``x = n[1:]``, ``pred = n[:-1]``) and one strided copy of the key frames; the decode is one launch per
non-key frame, in order, with the frame just restored as ``pred``.
"""

import numpy as np
import torch

from . import _device as dev
from . import _lib
from ._lib import check, lib

# the dtype of d for every sample dtype
SIGNED = {torch.uint8: torch.int8, torch.int8: torch.int8, torch.uint16: torch.int16, torch.int16: torch.int16,
          torch.int32: torch.int32}
NAMES = {'uint8': torch.uint8, 'int8': torch.int8, 'uint16': torch.uint16, 'int16': torch.int16,
         'int32': torch.int32}


def check_key_interval(key_interval):
    """``K`` as None or an int >= 1.  ValueError for a bool, anything that is not an int, or a value < 1."""
    if key_interval is None:
        return None
    if isinstance(key_interval, bool) or not isinstance(key_interval, (int, np.integer)) or key_interval < 1:
        raise ValueError(f'key_interval must be None or an int >= 1, got {key_interval!r}')
    return int(key_interval)


def is_key(t, key_interval):
    """Whether frame ``t`` is a key frame under the (checked) ``key_interval``."""
    return t == 0 or (key_interval is not None and t % key_interval == 0)


def sample_dtype(dtype, who='delta'):
    """The torch dtype of a sample dtype given as a torch dtype, a numpy dtype or its name.  TypeError for
    anything but uint8, int8, uint16, int16 and int32."""
    if isinstance(dtype, torch.dtype):
        dt = dtype
    else:
        try:
            dt = NAMES.get(np.dtype(dtype).name)
        except TypeError:
            dt = None
    if dt not in SIGNED:
        raise TypeError(f'{who}: delta coding takes uint8, int8, uint16, int16 or int32 samples, got {dtype!r}')
    return dt


def _input_dtype(x):
    return x.dtype if isinstance(x, torch.Tensor) else np.asarray(x).dtype


def _check_frames(x, who):
    if len(x.shape) < 1:
        raise ValueError(f'{who}: the array needs a leading time axis')


def _launch(direction, pred, x, out):
    check(lib.kmp_code(direction, _lib.CODER_DELTA, dev.dtype_code(x), pred.data_ptr(), dev.dtype_code(x), x.data_ptr(),
                       x.numel(), out.data_ptr(), dev.stream()), 'code')


def d_encode(n, key_interval=None):
    """``d`` (the signed dtype of ``n``'s width) of the contiguous device tensor ``n`` of shape ``(T, ...)``:
    one ``kmp_code`` launch over the frames 1 .. T-1, then the key frames copied over it."""
    K = key_interval
    assert n.is_contiguous()
    s = n.view(SIGNED[n.dtype])
    if n.shape[0] <= 1 or K == 1 or n[0].numel() == 0:  # key frames alone
        return s.clone()
    d = dev.empty(n.shape, s.dtype)
    _launch(_lib.ENCODE, s[:-1], s[1:], d[1:])
    if K is None:
        d[0].copy_(s[0])
    else:
        d[::K].copy_(s[::K])
    return d


def d_decode(d, key_interval=None, out=None):
    """``n`` (in ``d``'s dtype: the caller reinterprets it) of the contiguous device tensor ``d``: the key
    frames as they are, every other frame by one ``kmp_code`` launch with the frame just restored as ``pred``,
    in stream order.  ``out``: the result's tensor (``d`` itself is allowed), a new one by default."""
    K = key_interval
    if out is None:
        out = d.clone()
    elif out is not d:
        out.copy_(d)
    if d.shape[0] <= 1 or K == 1 or d[0].numel() == 0:
        return out
    # the frames by address: a launch per frame, so the host's share of each one counts
    assert out.is_contiguous()
    F, code, stream = out[0].numel(), dev.dtype_code(out), dev.stream()
    base, step = out.data_ptr(), out[0].numel() * out.element_size()
    for t in range(1, d.shape[0]):
        if not is_key(t, K):  # in place: kmp_code allows out == x
            at = base + t * step
            check(lib.kmp_code(_lib.DECODE, _lib.CODER_DELTA, code, at - step, code, at, F, at, stream), 'code')
    return out


def encode(n, key_interval=None):
    """``d`` for the integer array ``n`` of shape ``(T, ...)`` (uint8, int8, uint16, int16 or int32), in the
    signed dtype of its width.  numpy in gives numpy out, a CUDA tensor in gives a CUDA tensor out.  A dtype
    that is not one of the five is TypeError, a bad ``key_interval`` ValueError, both before the device is
    touched."""
    sample_dtype(_input_dtype(n), 'delta.encode')
    K = check_key_interval(key_interval)
    _check_frames(n, 'delta.encode')
    nt, kind = dev.to_device(n)
    return dev.from_device(d_encode(nt, K), kind)


def decode(d, dtype, key_interval=None):
    """The array ``encode`` was given: ``d`` (int8, int16 or int32) summed along the chain and reinterpreted
    as the sample ``dtype`` (a torch dtype, a numpy dtype or its name) of the same width."""
    dt = sample_dtype(dtype, 'delta.decode')
    have = sample_dtype(_input_dtype(d), 'delta.decode')
    if have != SIGNED[dt]:
        raise TypeError(f'delta.decode: the deltas of {dtype!r} samples are {SIGNED[dt]}, got {have}')
    K = check_key_interval(key_interval)
    _check_frames(d, 'delta.decode')
    t, kind = dev.to_device(d)
    return dev.from_device(d_decode(t, K).view(dt), kind)
