"""Near-lossless coding (``max_error``) -- a build extension with no reference counterpart
(DESIGN.md §16).

The caller states a bound ``max_error = d`` and every restored sample differs from the original by at
most ``d``.  Samples are uint8 / uint16 / int8 / int16, W bits wide (signed ones are coded on
``M(x) = x ^ signbit``); ``1 <= d <= 2^(W-1) - 1`` and ``step = 2 d + 1``.  For a prediction ``P``
clamped to the sample range and a sample ``x`` the map holds ``q = sign(e) ((|e| + d) // step)``,
``e = x - P``, as W-bit two's complement in the unsigned map dtype, and the decode returns
``clamp(P + q step)``.  ``max_error = 0`` is not a quantiser: it names the lossless modular coder.

:func:`coders` returns plain ``coder(pred, value)`` functions like those of ``kom.utils``; handed to
``kom.volume`` / ``kom.image`` ``encode`` / ``decode`` (and the chunked drivers) they run the fused
generic kernels for a built-in predictor and the two callback launches for an opaque
``predictions_fn``.  :func:`encode_pyramid` runs the closed loop over a pyramid -- each level is
predicted from the *reconstructed* coarser level, so the bound holds at the finest level -- and the
existing ``decode_pyramid`` with ``coders(...)[1]`` is its decoder.
"""

import numpy as np
import torch

from . import _device as dev
from . import _lib, _nd, _trace

_NEAR_CODE = {torch.uint8: _lib.CODER_NEAR_U8, torch.int8: _lib.CODER_NEAR_U8,
              torch.uint16: _lib.CODER_NEAR_U16, torch.int16: _lib.CODER_NEAR_U16}
_LOSSLESS = {torch.uint8: 'uint8', torch.uint16: 'uint16', torch.int8: 'int8', torch.int16: 'int16',
             torch.int32: 'raw', torch.uint32: 'uint32'}
_BY_NAME = {'uint8': torch.uint8, 'uint16': torch.uint16, 'int8': torch.int8, 'int16': torch.int16,
            'int32': torch.int32, 'uint32': torch.uint32, 'float32': torch.float32}
# torch has few kernels for uint16: strided copies of the plumbing run on the same-width signed view
_PLUMB = {torch.uint16: torch.int16}


def torch_dtype(dtype):
    """``dtype`` (torch, numpy or a name) as a torch dtype; TypeError for one that is no sample dtype."""
    if isinstance(dtype, torch.dtype):
        return dtype
    try:
        return _BY_NAME[np.dtype(dtype).name]
    except (TypeError, KeyError):
        raise TypeError(f'kompressor_amd.near: {dtype!r} is not a sample dtype') from None


def max_error_limit(dtype):
    """The largest ``max_error`` of a sample dtype: ``2^(W-1) - 1``."""
    return (1 << (8 * torch_dtype(dtype).itemsize - 1)) - 1


def check_max_error(dtype, max_error):
    """The arguments of a near-lossless request, checked on the host alone: ValueError for a
    ``max_error`` that is no int, negative or too large for the dtype; TypeError for 32-bit and float
    samples (``max_error > 0`` only: 0 is every dtype's lossless coder).  Returns the torch dtype."""
    if isinstance(max_error, bool) or not isinstance(max_error, (int, np.integer)):
        raise ValueError(f'max_error must be an int, got {max_error!r}')
    if max_error < 0:
        raise ValueError(f'max_error must be >= 0, got {max_error}')
    tdt = torch_dtype(dtype)
    if max_error == 0:
        return tdt
    if tdt not in _NEAR_CODE:
        raise TypeError(f'no near-lossless coder for {tdt} samples (uint8, uint16, int8, int16 only)')
    if max_error > max_error_limit(tdt):
        raise ValueError(f'max_error {max_error} is too large for {tdt}: at most {max_error_limit(tdt)}')
    return tdt


def coder_id(dtype, max_error):
    """The ``coder`` argument of the C-ABI for ``dtype`` samples under ``max_error`` (0: the natural
    lossless coder)."""
    tdt = check_max_error(dtype, max_error)
    if max_error == 0:
        if tdt not in _nd.NATURAL_CODER:
            raise TypeError(f'no lossless coder for {tdt}')
        return _nd.NATURAL_CODER[tdt]
    return _lib.coder_near(_NEAR_CODE[tdt], int(max_error))


def _near_fn(direction, coder, tdt, name, doc):
    x_code = dev.TORCH_TO_CODE[tdt]  # the sample dtype's code: it says whether the samples are signed
    map_dtype = _nd.CODER_DTYPE[coder]

    def fn(pred, x):
        kind = 'torch' if dev.is_torch(x) else 'numpy'
        xt = _nd._dev(x)
        want = tdt if direction == _lib.ENCODE else map_dtype
        if xt.dtype != want:
            raise TypeError(f'{name}: expected {want} values, got {xt.dtype}')
        pt = _nd._dev(pred)
        if pt.dtype not in (tdt, torch.float32):
            raise TypeError(f'{name}: predictions must be {tdt} or float32, got {pt.dtype}')
        out = _nd.d_code(direction, coder, pt, xt, x_code)
        return dev.from_device(out if direction == _lib.ENCODE else out.view(tdt), kind)

    fn.__name__ = fn.__qualname__ = name
    fn.__doc__ = doc
    fn._kmp_coder = (coder, direction)
    return fn


def coders(dtype, max_error):
    """``(encode_fn, decode_fn)`` for ``dtype`` samples with ``|restored - original| <= max_error``.
    ``max_error = 0`` returns the dtype's lossless pair of ``kom.utils``.  The decode function
    returns the sample dtype (the signed one for int8 / int16)."""
    tdt = check_max_error(dtype, max_error)
    if max_error == 0:
        from . import utils
        if tdt not in _LOSSLESS:
            raise TypeError(f'no lossless coder for {tdt}')
        return (getattr(utils, f'encode_values_{_LOSSLESS[tdt]}'), getattr(utils, f'decode_values_{_LOSSLESS[tdt]}'))
    coder = coder_id(tdt, max_error)
    tag = f'{_BY_NAME_INV[tdt]}_near{int(max_error)}'
    return (_near_fn(_lib.ENCODE, coder, tdt, f'encode_values_{tag}',
                     f'q = sign(e) ((|e| + {max_error}) // {2 * max_error + 1}), e = value - pred, as {tdt} bits.'),
            _near_fn(_lib.DECODE, coder, tdt, f'decode_values_{tag}',
                     f'clamp(pred + q * {2 * max_error + 1}) in {tdt}: within {max_error} of the coded value.'))


_BY_NAME_INV = {v: k for k, v in _BY_NAME.items()}


def _input_dtype(x):
    return x.dtype if isinstance(x, torch.Tensor) else np.asarray(x).dtype


def d_encode_pyramid(predictor, h, levels, coder):
    """The closed loop on a contiguous device tensor ``h`` with the near ``coder`` id: ``(lowres,
    [(maps, dims), ...] finest first, restored)``, device tensors.  The strided level views and the
    node replacement are torch plumbing; the coding is the fused encode and decode of each level,
    coarsest first, the decode giving the nodes of the next finer level."""
    ndim = predictor.ndim
    _nd._require(isinstance(levels, int) and not isinstance(levels, bool) and levels >= 1, 'levels must be an int >= 1')
    plumb = _PLUMB.get(h.dtype, h.dtype)
    hv = h.view(plumb)

    def level(k):
        return hv[(slice(None), *[slice(None, None, 2 ** k)] * ndim)]

    for k in range(levels):  # every level's highres is one the codec takes (as kom.container.compress checks)
        shape = level(k).shape
        sp = _nd._sp(shape, ndim)
        _nd.validate_highres_shape((shape[0], *[s + (s + 1) % 2 for s in sp], *shape[1 + ndim:]), ndim)
    r = level(levels).contiguous()
    lowres, out = r.view(h.dtype), [None] * levels
    for k in reversed(range(levels)):
        hk = level(k).clone(memory_format=torch.contiguous_format)
        hk[(slice(None), *[slice(None, None, 2)] * ndim)] = r
        hk = hk.view(h.dtype)
        lo, maps, dims = _nd._alloc_encoded(hk, coder, ndim)
        _nd.fused_encode_into(hk, predictor, coder, lo, maps, ndim)
        restored = dev.empty(hk.shape, h.dtype)
        _nd.fused_decode_into(lo, maps, dims, predictor, coder, restored, ndim)
        out[k] = (tuple(maps), tuple(dims))
        r = restored.view(plumb)
    return lowres, out, r.view(h.dtype)


@_trace.traced('kmp.near.encode_pyramid')
def encode_pyramid(predictor, highres, levels, max_error):
    """Closed-loop pyramid encode of ``highres`` with a built-in ``predictor``: ``(lowres, [(maps,
    dims), ...] finest first, restored)`` with ``|restored - highres| <= max_error`` everywhere and
    ``restored`` exactly what ``decode_pyramid(predictor, coders(dtype, max_error)[1], lowres,
    encoded)`` returns.  ``max_error = 0`` is the lossless pyramid (``restored`` equals ``highres``)."""
    tdt = check_max_error(_input_dtype(highres), max_error)
    if not hasattr(predictor, '_kmp_predictor'):
        raise TypeError('near.encode_pyramid takes a built-in predictor (MeanPredictor / LinearPredictor)')
    if max_error == 0:
        enc = coders(tdt, 0)[0]
        lowres, encoded = _nd.encode_pyramid(predictor, enc, highres, levels, predictor.padding, predictor.ndim)
        return lowres, encoded, highres
    h, kind = dev.to_device(highres)
    lowres, encoded, restored = d_encode_pyramid(predictor, h, levels, coder_id(tdt, max_error))
    return (dev.from_device(lowres, kind),
            [(tuple(dev.from_device(m, kind) for m in maps), dims) for maps, dims in encoded],
            dev.from_device(restored, kind))


def d_max_abs_error(a, b):
    """``max |a - b|`` of two device tensors of one 8- / 16-bit sample dtype, as a Python int (one
    read-back)."""
    def i32(t):
        if t.dtype == torch.uint16:
            return t.view(torch.int16).to(torch.int32) & 0xffff
        return t.to(torch.int32)
    if a.numel() == 0:
        return 0
    return int((i32(a) - i32(b)).abs().max().item())
