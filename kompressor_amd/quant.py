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

The relative mode (``rel_error``) is the second half of the module: ``mantissa_bits``,
``effective_rel``, ``quantise_rel``, ``restore_rel``.
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
    _require_quantised(n, exceptions, 'quant.restore')
    exp = check_exponent(exp)
    nt, kind = dev.to_device(n)
    return dev.from_device(d_restore(nt, exp, _device_exceptions(nt, exceptions, 'quant.restore')), kind)


def _require_quantised(n, exceptions, who):
    """TypeError unless ``n`` is int16 / int32 and ``exceptions`` None or (int64, uint32) arrays: no device work."""
    dt = _input_dtype(n)
    if dt not in (torch.int16, torch.int32, np.dtype(np.int16), np.dtype(np.int32)):
        raise TypeError(f'{who}: quantised values are int16 or int32, got {dt}')
    if exceptions is not None:
        idx, bits = exceptions
        if _input_dtype(idx) not in (torch.int64, np.dtype(np.int64)) or \
                _input_dtype(bits) not in (torch.uint32, np.dtype(np.uint32)):
            raise TypeError(f'{who}: exceptions are (int64 indices, uint32 bits)')


def _device_exceptions(nt, exceptions, who):
    """``exceptions`` on the device, checked against the device tensor ``nt`` they index (ValueError)."""
    if exceptions is None:
        return None
    idx, bits = exceptions
    it = idx.to('cuda') if isinstance(idx, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(idx)).to('cuda')
    bt = dev.to_device(bits)[0]
    if it.shape != bt.shape or it.dim() != 1:
        raise ValueError(f'{who}: indices and bits are two 1-d arrays of one length')
    if it.numel() and (int(it.min().item()) < 0 or int(it.max().item()) >= nt.numel()):
        raise ValueError(f'{who}: an exception index lies outside the array')
    return it, bt


# ---------------------------------------------------------------------------------------------
# the relative mode (``rel_error``): keep the top m mantissa bits of every float32
# ---------------------------------------------------------------------------------------------
# With ``mant, ex = frexp(rel_error)``: ``m = -ex``, ``t = 23 - m`` and the bound kept is
# ``eps_rel = 2**-(m + 1)``, so ``rel_error / 2 < eps_rel <= rel_error``.  On the bits ``u`` of a float32,
# ``a = u & 0x7fffffff``, in 32-bit unsigned arithmetic:
#
#     k = (a + 2**(t-1) - 1 + ((a >> t) & 1)) >> t        round to nearest, ties to even
#     x is an exception  iff  a >= 0x7f800000 or (k << t) >= 0x7f800000 or k > QMAX
#     n = -k if the sign bit is set else k
#
# and a non-exception restores to the float32 of bits ``(|n| << t) | sign``, within
# ``eps_rel * max(|x|, 2**-126)`` of ``x``.  The arithmetic is ``kmp_code`` with the
# ``KMP_CODER_PREC_I16 / _I32`` coders; exceptions travel as for the absolute mode.

M_MIN, M_MAX = 0, 22
_M_ALWAYS_I16 = 7  # |n| <= 255 * 2**m - 1, which is 32639 at m = 7: int16 whatever the data
_PREC_CODE = {torch.int16: _lib.CODER_PREC_I16, torch.int32: _lib.CODER_PREC_I32}


def mantissa_bits(rel_error):
    """``m``, the mantissa bits kept under the relative bound ``rel_error``.  ValueError for a bool, a
    string, a value that is not finite or not positive, ``>= 1``, or below ``2**-23`` (code such data
    lossless)."""
    if isinstance(rel_error, (bool, str, bytes)) or not isinstance(rel_error, (int, float, np.integer, np.floating)):
        raise ValueError(f'rel_error must be a number in [2**-23, 1), got {rel_error!r}')
    try:
        a = float(rel_error)
    except OverflowError:
        a = math.inf
    if not math.isfinite(a) or a <= 0:
        raise ValueError(f'rel_error must be a number in [2**-23, 1), got {rel_error!r}')
    m = -math.frexp(a)[1]
    if not M_MIN <= m <= M_MAX:
        raise ValueError(f'rel_error {rel_error!r} is outside [2**-23, 1)')
    return m


def effective_rel(rel_error):
    """The relative bound actually kept, ``2**-(mantissa_bits(rel_error) + 1)``: in ``(rel_error / 2, rel_error]``."""
    return math.ldexp(1.0, -(mantissa_bits(rel_error) + 1))


def check_mantissa_bits(bits):
    if isinstance(bits, bool) or not isinstance(bits, (int, np.integer)) or not M_MIN <= bits <= M_MAX:
        raise ValueError(f'the kept mantissa bits must be an int in [{M_MIN}, {M_MAX}], got {bits!r}')
    return int(bits)


def d_code_rel(direction, dtype, bits, x):
    """One ``kmp_code`` launch of the relative quantiser of integer ``dtype`` on the contiguous device
    tensor ``x``: float32 -> ``dtype`` with the sentinel at the exceptions (ENCODE), ``dtype`` -> float32 (DECODE)."""
    out = dev.empty(x.shape, dtype if direction == _lib.ENCODE else torch.float32)
    if x.numel():
        check(lib.kmp_code(direction, _lib.coder_prec(_PREC_CODE[dtype], bits), 0, None, dev.dtype_code(x),
                           x.data_ptr(), x.numel(), out.data_ptr(), dev.stream()), 'code')
    return out


def d_quantise_rel(x, bits):
    """``(n, exceptions)`` of the contiguous device float32 tensor ``x`` with ``bits`` mantissa bits kept:
    as :func:`d_quantise`.  Up to 7 bits every ``n`` fits int16, so that launch is the only one."""
    first = torch.int16 if bits <= _M_ALWAYS_I16 else torch.int32
    n = d_code_rel(_lib.ENCODE, first, bits, x)
    mask = n == _SENTINEL[first]
    n.masked_fill_(mask, 0)
    if first == torch.int32 and (x.numel() == 0 or int(n.abs().max().item()) <= _I16_MAX):
        # every non-exception fits int16: the kernel again on that type (the same exception set)
        n = d_code_rel(_lib.ENCODE, torch.int16, bits, x)
        mask = n == _SENTINEL[torch.int16]
        n.masked_fill_(mask, 0)
    idx = mask.reshape(-1).nonzero().reshape(-1)
    if idx.numel() == 0:
        return n, None
    return n, (idx, x.reshape(-1).view(torch.int32)[idx].view(torch.uint32))


def d_restore_rel(n, bits, exceptions):
    """The float32 device tensor of the bits ``|n| << (23 - bits)`` and ``n``'s sign, the exceptions' bits put back."""
    out = d_code_rel(_lib.DECODE, n.dtype, bits, n)
    if exceptions is not None:
        idx, raw = exceptions
        out.reshape(-1).view(torch.int32)[idx] = raw.view(torch.int32)
    return out


def quantise_rel(x, rel_error):
    """``(n, exceptions)`` for float32 ``x`` under the pointwise relative bound ``rel_error``, with the
    conventions of :func:`quantise`: ``n`` int16 when every quantised value fits it and int32 otherwise,
    0 at the exceptions (not finite, or rounding up to infinity); ``exceptions`` None or ``(int64 flat
    indices ascending, uint32 bits)``.  ``n`` is monotone in ``x``."""
    _require_f32(x, 'quant.quantise_rel')
    bits = mantissa_bits(rel_error)
    xt, kind = dev.to_device(x)
    n, exc = d_quantise_rel(xt, bits)
    if exc is not None:
        exc = (dev.from_device(exc[0], kind), dev.from_device(exc[1], kind))
    return dev.from_device(n, kind), exc


def restore_rel(n, bits, exceptions=None):
    """The float32 array ``quantise_rel`` stands for, ``bits = mantissa_bits(rel_error)``: every
    non-exception within ``2**-(bits + 1) * max(|x|, 2**-126)`` of its original, the exceptions bit for bit."""
    _require_quantised(n, exceptions, 'quant.restore_rel')
    bits = check_mantissa_bits(bits)
    nt, kind = dev.to_device(n)
    return dev.from_device(d_restore_rel(nt, bits, _device_exceptions(nt, exceptions, 'quant.restore_rel')), kind)


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
