"""Error-bounded float32 coding (``abs_error``) -- a build extension with no reference counterpart
(DESIGN.md §17).

The caller states an absolute bound and gets integers the whole lossless machinery codes (fused
codec, pyramids, Rice bundles, partial reads), plus the few values that cannot be quantised.  The
step is the power of two ``2**e`` with ``m, e = frexp(abs_error)`` and the bound kept is
``eps = 2**(e - 1)``, so ``abs_error / 2 < eps <= abs_error``.  With ``QMAX`` = 32767 (int16) or
2^31 - 1 (int32), in float64::

    n = rint(x * 2**-e)                     ties to even
    r = float32(n * 2**e)
    x is an exception  iff  x is not finite, |n| > QMAX, r is not finite or |r - x| > eps

A non-exception restores to ``r``; an exception is carried as its raw 32 bits and restores bit for
bit.  The arithmetic is ``kmp_code`` with the ``KMP_CODER_QUANT_I16 / _I32`` coders; an array is int16
when every non-exception fits it, else int32.
"""

import math

import numpy as np
import torch

from . import _device as dev
from . import _lib, _nd
from ._lib import check, lib

E_MIN, E_MAX = -126, 127
_CODE = {torch.int16: _lib.CODER_QUANT_I16, torch.int32: _lib.CODER_QUANT_I32}
_SENTINEL = {torch.int16: -(1 << 15), torch.int32: -(1 << 31)}
_I16_MAX = (1 << 15) - 1


def exponent(abs_error):
    """``e`` of the step ``2**e`` for the bound ``abs_error``.  ValueError for a bool, a string, a value
    that is not finite or not positive, or an exponent outside [-126, 127]."""
    if isinstance(abs_error, (bool, str, bytes)) or not isinstance(abs_error, (int, float, np.integer, np.floating)):
        raise ValueError(f'abs_error must be a positive finite number, got {abs_error!r}')
    try:
        a = float(abs_error)
    except OverflowError:
        a = math.inf
    if not math.isfinite(a) or a <= 0:
        raise ValueError(f'abs_error must be a positive finite number, got {abs_error!r}')
    e = math.frexp(a)[1]
    if not E_MIN <= e <= E_MAX:
        raise ValueError(f'abs_error {abs_error!r}: the step 2**{e} is outside 2**{E_MIN} .. 2**{E_MAX}')
    return e


def effective(abs_error):
    """The bound actually kept, ``2**(exponent(abs_error) - 1)``: in ``(abs_error / 2, abs_error]``."""
    return math.ldexp(1.0, exponent(abs_error) - 1)


def check_exponent(exp):
    if isinstance(exp, bool) or not isinstance(exp, (int, np.integer)) or not E_MIN <= exp <= E_MAX:
        raise ValueError(f'the step exponent must be an int in [{E_MIN}, {E_MAX}], got {exp!r}')
    return int(exp)


def _input_dtype(x):
    return x.dtype if isinstance(x, torch.Tensor) else np.asarray(x).dtype


def _require_f32(x, who):
    dt = _input_dtype(x)
    if dt not in (torch.float32, np.dtype(np.float32)):
        raise TypeError(f'{who}: error-bounded coding takes float32 samples, got {dt}')


def d_code(direction, dtype, exp, x):
    """One ``kmp_code`` launch of the quantiser of integer ``dtype`` on the contiguous device tensor
    ``x``: float32 -> ``dtype`` with the sentinel at the exceptions (ENCODE), ``dtype`` -> float32 (DECODE)."""
    out = dev.empty(x.shape, dtype if direction == _lib.ENCODE else torch.float32)
    if x.numel():
        check(lib.kmp_code(direction, _lib.coder_quant(_CODE[dtype], exp), 0, None, dev.dtype_code(x), x.data_ptr(),
                           x.numel(), out.data_ptr(), dev.stream()), 'code')
    return out


def d_quantise(x, exp):
    """``(n, exceptions)`` of the contiguous device float32 tensor ``x``: ``n`` int16 / int32 with 0 at
    the exceptions, ``exceptions`` None or ``(flat int64 indices ascending, uint32 bits)`` on the device."""
    n = d_code(_lib.ENCODE, torch.int32, exp, x)
    mask = n == _SENTINEL[torch.int32]
    n.masked_fill_(mask, 0)
    if x.numel() == 0 or int(n.abs().max().item()) <= _I16_MAX:
        # every non-exception fits int16: the kernel again on that type (the same exception set)
        n = d_code(_lib.ENCODE, torch.int16, exp, x)
        mask = n == _SENTINEL[torch.int16]
        n.masked_fill_(mask, 0)
    idx = mask.reshape(-1).nonzero().reshape(-1)
    if idx.numel() == 0:
        return n, None
    return n, (idx, x.reshape(-1).view(torch.int32)[idx].view(torch.uint32))


def d_restore(n, exp, exceptions):
    """The float32 device tensor ``n * 2**exp`` with the exceptions' bits put back."""
    out = d_code(_lib.DECODE, n.dtype, exp, n)
    if exceptions is not None:
        idx, bits = exceptions
        out.reshape(-1).view(torch.int32)[idx] = bits.view(torch.int32)
    return out


def quantise(x, abs_error):
    """``(n, exceptions)`` for float32 ``x`` under the bound ``abs_error``: ``n`` is int16 when every
    quantised value fits it and int32 otherwise, 0 where ``x`` is an exception; ``exceptions`` is None
    when there are none, else ``(index, bits)`` sorted by flat C-order index (int64 indices, the uint32
    bit patterns).  numpy in gives numpy out, a CUDA tensor in gives CUDA tensors out.  ``n`` is an
    ordinary integer array: the lossless ``encode`` of its dtype and ``packing`` take it as it is."""
    _require_f32(x, 'quant.quantise')
    exp = exponent(abs_error)
    xt, kind = dev.to_device(x)
    n, exc = d_quantise(xt, exp)
    if exc is not None:
        exc = (dev.from_device(exc[0], kind), dev.from_device(exc[1], kind))
    return dev.from_device(n, kind), exc


def restore(n, exp, exceptions=None):
    """The float32 array ``quantise`` stands for: ``float32(n * 2**exp)``, the exceptions bit for bit."""
    dt = _input_dtype(n)
    if dt not in (torch.int16, torch.int32, np.dtype(np.int16), np.dtype(np.int32)):
        raise TypeError(f'quant.restore: quantised values are int16 or int32, got {dt}')
    exp = check_exponent(exp)
    if exceptions is not None:
        idx, bits = exceptions
        if _input_dtype(idx) not in (torch.int64, np.dtype(np.int64)) or \
                _input_dtype(bits) not in (torch.uint32, np.dtype(np.uint32)):
            raise TypeError('quant.restore: exceptions are (int64 indices, uint32 bits)')
    nt, kind = dev.to_device(n)
    if exceptions is not None:
        it = idx.to('cuda') if isinstance(idx, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(idx)).to('cuda')
        bt = dev.to_device(bits)[0]
        if it.shape != bt.shape or it.dim() != 1:
            raise ValueError('quant.restore: indices and bits are two 1-d arrays of one length')
        if it.numel() and (int(it.min().item()) < 0 or int(it.max().item()) >= nt.numel()):
            raise ValueError('quant.restore: an exception index lies outside the array')
        exceptions = (it, bt)
    return dev.from_device(d_restore(nt, exp, exceptions), kind)


# ---------------------------------------------------------------------------------------------
# the container's exception arrays: gaps between consecutive sorted indices as two uint32 words
# ---------------------------------------------------------------------------------------------

def d_gaps(idx):
    """``(low words, high words)`` (uint32 device tensors) of the gaps between consecutive sorted int64
    indices, the first gap being the first index."""
    g = idx.clone()
    g[1:] -= idx[:-1]
    return _low32(g), _low32(g >> 32)


def _low32(v):
    """The low 32 bits of every int64 as uint32."""
    return v.view(torch.int32)[::2].contiguous().view(torch.uint32)


def d_indices(lo, hi):
    """The int64 indices of two uint32 gap-word tensors."""
    g = (lo.view(torch.int32).to(torch.int64) & 0xffffffff) | (hi.view(torch.int32).to(torch.int64) << 32)
    return torch.cumsum(g, 0)
