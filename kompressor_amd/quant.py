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
``effective_rel``, ``quantise_rel``, ``restore_rel``.  Masked fields are the last part:
``runs``, ``exceptions_from_runs``, ``fill`` and the device functions the container builds on.
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


def _d_int16_or_int32(encode, x, first, marks):
    """``(n, exception mask)`` of a quantiser ``encode(dtype)``: ``first`` tried, int16 when every
    non-exception fits it; 0 at the exceptions, or (``marks``) the type's minimum as ENCODE wrote it."""
    n = encode(first)
    mask = n == _SENTINEL[first]
    if not marks:
        n.masked_fill_(mask, 0)
    if first == torch.int32 and (x.numel() == 0 or
                                 int((n.masked_fill(mask, 0) if marks else n).abs().max().item()) <= _I16_MAX):
        # every non-exception fits int16: the kernel again on that type (the same exception set)
        n = encode(torch.int16)
        mask = n == _SENTINEL[torch.int16]
        if not marks:
            n.masked_fill_(mask, 0)
    return n, mask


def d_quantise(x, exp, marks=False):
    """``(n, exceptions)`` of the contiguous device float32 tensor ``x``: ``n`` int16 / int32 with 0 at
    the exceptions (``marks``: with the type's minimum there, for :func:`d_fill`), ``exceptions`` None or
    ``(flat int64 indices ascending, uint32 bits)`` on the device."""
    n, mask = _d_int16_or_int32(lambda dt: d_code(_lib.ENCODE, dt, exp, x), x, torch.int32, marks)
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


def d_quantise_rel(x, bits, marks=False):
    """``(n, exceptions)`` of the contiguous device float32 tensor ``x`` with ``bits`` mantissa bits kept:
    as :func:`d_quantise`.  Up to 7 bits every ``n`` fits int16, so that launch is the only one."""
    first = torch.int16 if bits <= _M_ALWAYS_I16 else torch.int32
    n, mask = _d_int16_or_int32(lambda dt: d_code_rel(_lib.ENCODE, dt, bits, x), x, first, marks)
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


# ---------------------------------------------------------------------------------------------
# masked fields: exceptions as runs, and the hold-fill of the integers under them
# ---------------------------------------------------------------------------------------------
# A run is a maximal stretch of consecutive flat indices whose bits are all equal, none longer than
# 2**32 - 1.  Stored: the low and high words of the gaps between consecutive run starts (the first gap is
# the first start), the lengths, and the differences of consecutive runs' bits modulo 2**32 (the first
# is the first run's bits) -- four uint32 arrays of R entries.  The fill gives every exception's
# integer the last non-exception's before it (the first one's in a leading stretch, 0 with none): the
# decoder overwrites those values from the runs, so any value serves and this one costs the pyramid least.

RUN_CAP = (1 << 32) - 1


def d_fill(n, out=None):
    """The hold-fill of the contiguous int16 / int32 device tensor ``n``, whose exceptions hold the type's
    minimum (as ``kmp_code`` ENCODE of a quantiser writes them): one ``kmp_code`` call (KMP_CODER_FILL).
    ``out``: the result's tensor (``n`` itself is allowed), a new one by default."""
    out = dev.empty(n.shape, n.dtype) if out is None else out
    if n.numel():
        ws = dev.empty((_lib.FILL_BYTES,), torch.uint8)
        check(lib.kmp_code(_lib.ENCODE, _lib.CODER_FILL, 0, ws.data_ptr(), dev.dtype_code(n), n.data_ptr(), n.numel(),
                           out.data_ptr(), dev.stream()), 'code')
    return out


def d_mark(n, exceptions):
    """``n`` itself with the type's minimum written at the ``exceptions`` (in place): what ENCODE wrote."""
    if exceptions is not None:
        n.reshape(-1)[exceptions[0]] = _SENTINEL[n.dtype]
    return n


def _cut(starts, lengths, bits, piece):
    """Runs no longer than ``piece``: every longer one cut into pieces from its start (int64 tensors)."""
    if starts.numel() == 0 or int(lengths.max().item()) <= piece:
        return starts, lengths, bits
    k = (lengths + (piece - 1)) // piece
    rep = torch.repeat_interleave(torch.arange(k.numel(), device=k.device), k)
    first = torch.cumsum(k, 0) - k
    at = (torch.arange(rep.numel(), device=k.device) - first[rep]) * piece
    return starts[rep] + at, torch.clamp(lengths[rep] - at, max=piece), bits[rep]


def d_run_list(idx, bits, cap=RUN_CAP):
    """``(starts, lengths, bits)`` (int64 device tensors, the bits in [0, 2**32)) of the runs of the sorted
    int64 indices ``idx`` and their uint32 ``bits``."""
    b = bits.view(torch.int32)
    new = torch.ones(idx.shape, dtype=torch.bool, device=idx.device)
    new[1:] = ((idx[1:] - idx[:-1]) != 1) | (b[1:] != b[:-1])
    first = new.nonzero().reshape(-1)
    lengths = torch.diff(first, append=torch.tensor([idx.numel()], device=idx.device))
    return _cut(idx[first], lengths, b[first].to(torch.int64) & 0xffffffff, cap)


def d_runs(idx, bits):
    """``(start gaps low, high, lengths, bit deltas)`` (uint32 device tensors) of the exceptions ``(idx, bits)``."""
    starts, lengths, rb = d_run_list(idx, bits)
    delta = rb.clone()
    delta[1:] -= rb[:-1]
    return (*d_gaps(starts), _low32(lengths), _low32(delta))


def d_run_starts(lo, hi, lengths, delta):
    """``(starts, lengths, bits)`` (int64 device tensors, the bits in [0, 2**32)) of the four stored arrays."""
    def wide(v):
        return v.view(torch.int32).to(torch.int64) & 0xffffffff
    return d_indices(lo, hi), wide(lengths), torch.cumsum(wide(delta), 0) & 0xffffffff


def d_check_runs(starts, lengths, numel):
    """ValueError unless every run has ``length >= 1`` and lies inside ``[0, numel)`` and the runs ascend
    without overlap: one read-back.  No sum of a start and a length is formed before the start is known to
    be inside the array, so a start near 2**63 (a damaged file's gap words reach any int64) cannot wrap
    past the comparison: ``numel - start`` is exact for ``0 <= start``, and the difference of two
    starts is exact once both lie in ``[0, numel]``."""
    if starts.numel():
        ok = (starts >= 0) & (lengths >= 1) & (lengths <= numel - starts)
        # only read where both neighbours are inside: elsewhere ``ok`` already fails
        ordered = (starts[1:] - starts[:-1]) >= lengths[:-1]
        if not bool((ok.all() & ordered.all()).item()):
            raise ValueError('an exception run is empty, lies outside the array or overlaps another')


def d_table(starts, lengths, bits, piece=_lib.RUNS_PIECE):
    """The ``(R', 4)`` uint32 device table of KMP_CODER_RUNS -- start low, start high, length, bits per
    record -- of checked runs, every run longer than ``piece`` cut into records of at most ``piece``."""
    starts, lengths, bits = _cut(starts, lengths, bits, piece)
    cols = [_low32(starts), _low32(starts >> 32), _low32(lengths), _low32(bits)]
    return torch.stack([c.view(torch.int32) for c in cols], 1).contiguous().view(torch.uint32)


def d_run_table(lo, hi, lengths, delta, numel, piece=_lib.RUNS_PIECE):
    """:func:`d_table` of the four stored arrays, the runs' extents checked against ``numel`` first."""
    runs_ = d_run_starts(lo, hi, lengths, delta)
    d_check_runs(runs_[0], runs_[1], numel)
    return d_table(*runs_, piece)


def d_patch_runs(out, table):
    """The contiguous float32 device tensor ``out`` patched in place from ``table`` (:func:`d_run_table`, whose
    check is what keeps the writes inside ``out``): one ``kmp_code`` call (KMP_CODER_RUNS)."""
    if table.shape[0]:
        check(lib.kmp_code(_lib.DECODE, _lib.CODER_RUNS, 0, None, _lib.U32, table.data_ptr(), table.shape[0],
                           out.data_ptr(), dev.stream()), 'code')
    return out


def d_expand(starts, lengths, bits):
    """``(int64 indices ascending, uint32 bits)`` of runs (int64 tensors, as :func:`d_run_starts`)."""
    rep = torch.repeat_interleave(torch.arange(starts.numel(), device=starts.device), lengths)
    first = torch.cumsum(lengths, 0) - lengths
    idx = starts[rep] + torch.arange(rep.numel(), device=starts.device) - first[rep]
    return idx, _low32(bits[rep])


def _require_runs(arrays, who):
    """TypeError / ValueError unless ``arrays`` are four 1-d uint32 arrays of one length: no device work."""
    if len(arrays) != 4:
        raise ValueError(f'{who}: runs are four arrays (start gaps low, high, lengths, bit deltas)')
    for a in arrays:
        if _input_dtype(a) not in (torch.uint32, np.dtype(np.uint32)):
            raise TypeError(f'{who}: the run arrays are uint32')
    if any(len(a.shape) != 1 or a.shape != arrays[0].shape for a in arrays):
        raise ValueError(f'{who}: the run arrays are 1-d and of one length')


def _require_exceptions(exceptions, who):
    idx, bits = exceptions
    if _input_dtype(idx) not in (torch.int64, np.dtype(np.int64)) or \
            _input_dtype(bits) not in (torch.uint32, np.dtype(np.uint32)):
        raise TypeError(f'{who}: exceptions are (int64 indices, uint32 bits)')
    if len(idx.shape) != 1 or idx.shape != bits.shape:
        raise ValueError(f'{who}: indices and bits are two 1-d arrays of one length')


def _index_tensor(idx):
    return idx.to('cuda') if isinstance(idx, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(idx)).to('cuda')


def runs(exceptions):
    """The stored form ``(start gaps low, high, lengths, bit deltas)`` -- four uint32 arrays -- of the
    ``exceptions`` ``(int64 indices ascending, uint32 bits)`` that ``quantise`` / ``quantise_rel`` return.
    numpy in gives numpy out, CUDA tensors in give CUDA tensors out."""
    _require_exceptions(exceptions, 'quant.runs')
    kind = 'torch' if isinstance(exceptions[0], torch.Tensor) else 'numpy'
    dev.require_gpu()
    out = d_runs(_index_tensor(exceptions[0]), dev.to_device(exceptions[1])[0])
    return tuple(dev.from_device(a, kind) for a in out)


def exceptions_from_runs(lo, hi, lengths, delta):
    """``(int64 indices ascending, uint32 bits)``: the runs of :func:`runs` expanded.  A run of length 0
    is ValueError."""
    arrays = (lo, hi, lengths, delta)
    _require_runs(arrays, 'quant.exceptions_from_runs')
    kind = 'torch' if isinstance(lo, torch.Tensor) else 'numpy'
    starts, lens, bits = d_run_starts(*[dev.to_device(a)[0] for a in arrays])
    if lens.numel() and int(lens.min().item()) < 1:
        raise ValueError('quant.exceptions_from_runs: a run of length 0')
    idx, b = d_expand(starts, lens, bits)
    return dev.from_device(idx, kind), dev.from_device(b, kind)


def fill(n, exceptions=None):
    """``n`` (int16 / int32, as ``quantise`` returns it) with the value at every exception replaced by the
    last non-exception's before it in flat C order -- the first one's before the first, 0 with none.
    ``restore`` of the result with the same exceptions is ``restore`` of ``n``."""
    _require_quantised(n, exceptions, 'quant.fill')
    if exceptions is not None:
        _require_exceptions(exceptions, 'quant.fill')
    nt, kind = dev.to_device(n)
    exc = _device_exceptions(nt, exceptions, 'quant.fill')
    if exc is None:
        return dev.from_device(nt, kind)
    return dev.from_device(d_fill(d_mark(nt.clone(), exc)), kind)
