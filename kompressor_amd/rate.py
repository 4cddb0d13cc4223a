"""Rate control (``target_bits`` / ``target_ratio``), the host side -- a build extension with no
reference counterpart.

A caller states a size instead of a bound; ``container.compress`` then picks, from a LADDER of bounds
running from the finest to the coarsest, the finest rung whose file fits the budget, sizing each
candidate on the device (``container.compressed_size``: the quantiser, the pyramid and the measuring
launches of the Rice bundle -- nothing written, no bundle allocated), and writes that rung with the
explicit-bound path.  Everything here is pure host arithmetic: the budget, the ladders and the search.

Ladders (``mode``):

* ``'abs'`` (float32): step exponents ``e``, i.e. ``abs_error = 2**(e - 1)``.  With ``M`` the largest
  finite ``|x|`` and ``ex = frexp(M)[1]``: ``e = clamp(ex - 30) .. clamp(ex + 1)``, clamped to
  ``[quant.E_MIN, quant.E_MAX]``.  At ``ex + 1`` every finite value quantises to 0 (``|x| * 2**-e <
  1/2``); at ``ex - 30`` the step is below the ulp of the largest values (``2**(ex - 24)``).  ``M = 0``
  or no finite value: the single rung ``e = 0``.
* ``'rel'`` (float32): kept mantissa bits ``m = 22 .. 0``, i.e. ``rel_error = 2**-(m + 1)``.
* ``'near'`` (uint8 / uint16 / int8 / int16): ``max_error = 0 .. near.max_error_limit(dtype)``.

The search assumes nothing about the sizes being monotone in the rung: it returns a rung that fits
whose finer neighbour does not (or rung 0), after at most ``2 + ceil(log2 L)`` probes.

A quality target (``target_psnr``) runs over the same ladders the other way round:
:func:`search_quality` returns a rung that meets the target whose coarser neighbour does not.
``target_ssim`` is the same search with the mean SSIM as the quality.
"""

import math

import numpy as np

from . import near, quant

MODES = {'float32': ('abs', 'rel'), 'uint8': ('near',), 'uint16': ('near',), 'int8': ('near',), 'int16': ('near',)}


def _positive_finite(name, v):
    if isinstance(v, (bool, str, bytes)) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise ValueError(f'{name} must be a positive finite number, got {v!r}')
    try:
        f = float(v)
    except OverflowError:
        f = math.inf
    if not math.isfinite(f) or f <= 0:
        raise ValueError(f'{name} must be a positive finite number, got {v!r}')
    return f


def check_target(dtype, target_bits, target_ratio, target_mode, method='rice', max_error=0, abs_error=None,
                 rel_error=None, target_psnr=None, target_ssim=None):
    """The arguments of a rate- or quality-controlled ``compress``, checked on the host alone.  Returns None
    when no target is given (``target_mode`` must then be None too), else the mode: the dtype's default or
    ``target_mode``.  ValueError: more than one target, a target that is no positive finite number, a
    ``target_ssim`` above 1, a target together with a bound, a size target with a method other than 'rice', an
    unknown mode or one that does not fit the dtype; TypeError: a sample dtype without a lossy mode."""
    targets = {'target_bits': target_bits, 'target_ratio': target_ratio, 'target_psnr': target_psnr,
               'target_ssim': target_ssim}
    given = [k for k, v in targets.items() if v is not None]
    if not given:
        if target_mode is not None:
            raise ValueError('target_mode needs target_bits, target_ratio or target_psnr')
        return None
    if len(given) > 1:
        if target_ssim is not None:
            raise ValueError(f'target_ssim stands alone among the targets, not with {" and ".join(given[:-1])}')
        raise ValueError(f'give one of target_bits, target_ratio and target_psnr, not {" and ".join(given)}')
    if _positive_finite(given[0], targets[given[0]]) > 1 and target_ssim is not None:
        raise ValueError(f'target_ssim must lie in (0, 1], got {target_ssim!r}')
    if isinstance(max_error, bool) or max_error != 0 or abs_error is not None or rel_error is not None:
        raise ValueError(f'{given[0]} chooses the bound: not with max_error, abs_error or rel_error')
    if target_psnr is None and target_ssim is None and method != 'rice':
        raise ValueError("target_bits / target_ratio need method='rice' (only Rice bundles are sized on the device)")
    try:
        name = near._BY_NAME_INV[near.torch_dtype(dtype)]
    except (TypeError, KeyError):
        name = None
    if name not in MODES:
        raise TypeError(f'no rate or quality control for {dtype} samples (float32: abs / rel; uint8, uint16, int8, int16: near)')
    every = tuple(m for ms in MODES.values() for m in ms)
    if target_mode is None:
        return MODES[name][0]
    if target_mode not in every:
        raise ValueError(f'unknown target_mode {target_mode!r} (expected one of {sorted(set(every))})')
    if target_mode not in MODES[name]:
        raise ValueError(f'target_mode {target_mode!r} does not fit {name} samples ({" / ".join(MODES[name])})')
    return target_mode


def budget_bytes(numel, raw_bytes, target_bits=None, target_ratio=None):
    """``floor(target_bits * numel / 8)`` or ``floor(raw_bytes / target_ratio)``."""
    if target_bits is not None:
        return int(math.floor(_positive_finite('target_bits', target_bits) * numel / 8))
    return int(math.floor(raw_bytes / _positive_finite('target_ratio', target_ratio)))


def ladder_abs(M):
    """The step exponents of the 'abs' ladder, finest first, for the largest finite magnitude ``M``
    (0, or not finite: no finite value to go by -- the single rung 0)."""
    M = float(M)
    if not math.isfinite(M) or M <= 0:
        return [0]

    def clamp(e):
        return min(max(e, quant.E_MIN), quant.E_MAX)
    ex = math.frexp(M)[1]
    return list(range(clamp(ex - 30), clamp(ex + 1) + 1))


def ladder_rel():
    """The kept mantissa bits of the 'rel' ladder, finest first."""
    return list(range(quant.M_MAX, quant.M_MIN - 1, -1))


def ladder_near(dtype):
    """The ``max_error`` values of the 'near' ladder, finest (0: lossless) first."""
    return range(0, near.max_error_limit(dtype) + 1)


def bound_of(mode, rung):
    """The ``compress`` keyword and value that code a ladder's rung value."""
    if mode == 'abs':
        return 'abs_error', math.ldexp(1.0, rung - 1)
    if mode == 'rel':
        return 'rel_error', math.ldexp(1.0, -(rung + 1))
    return 'max_error', int(rung)


class Unreachable(ValueError):
    """No rung of the ladder fits the budget; ``coarsest`` is the size of the coarsest one.  From
    :func:`search_quality`: no rung reaches the quality ``target``; ``finest`` is the finest one's."""

    def __init__(self, coarsest, budget):
        super().__init__(f'the budget of {budget} bytes cannot be met: the coarsest rung needs {coarsest} bytes '
                         f'(bound_bytes)')
        self.coarsest, self.budget = coarsest, budget

    @classmethod
    def quality(cls, finest, target):
        e = cls(None, None)
        e.args = (f'the quality target of {target} cannot be met: the finest rung reaches {finest}',)
        e.finest, e.target = finest, target
        return e


def search(size, L, budget):
    """``(rung, probes)``: the rung in ``0 .. L - 1`` (0 the finest) to code under ``budget`` bytes, with
    ``size(r)`` the bytes of rung ``r`` and ``probes`` the ``[(r, size(r))]`` asked, in order.

    1. ``size(0) <= budget``: rung 0.
    2. else ``size(L - 1) > budget``: :class:`Unreachable` (a ValueError).
    3. else bisect with ``lo = 0`` (too big) and ``hi = L - 1`` (fits): ``mid = (lo + hi) // 2`` goes to
       ``hi`` when it fits, else to ``lo``; stop at ``hi - lo == 1`` and take ``hi``.
    """
    probes = []

    def ask(r):
        probes.append((r, int(size(r))))
        return probes[-1][1]
    if ask(0) <= budget:
        return 0, probes
    if L == 1:
        raise Unreachable(probes[0][1], budget)
    coarsest = ask(L - 1)
    if coarsest > budget:
        raise Unreachable(coarsest, budget)
    lo, hi = 0, L - 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if ask(mid) <= budget:
            hi = mid
        else:
            lo = mid
    return hi, probes


def search_quality(quality, L, target):
    """``(rung, probes)``: the rung in ``0 .. L - 1`` (0 the finest) to code for a quality of at least
    ``target``, with ``quality(r)`` the figure of rung ``r`` (a PSNR in dB) and ``probes`` the
    ``[(r, quality(r))]`` asked, in order.

    1. ``quality(L - 1) >= target``: rung ``L - 1``.
    2. else ``quality(0) < target``: :class:`Unreachable` (``finest`` holds rung 0's quality).
    3. else bisect with ``lo = 0`` (meets the target) and ``hi = L - 1`` (fails): ``mid = (lo + hi) // 2``
       goes to ``lo`` when it meets the target, else to ``hi``; stop at ``hi - lo == 1`` and take ``lo``.

    Nothing is assumed about the quality being monotone in the rung: the rung returned meets the target,
    its coarser neighbour does not (or does not exist), after at most ``2 + ceil(log2 L)`` probes."""
    probes = []

    def ask(r):
        probes.append((r, float(quality(r))))
        return probes[-1][1]
    if ask(L - 1) >= target:
        return L - 1, probes
    if L == 1:
        raise Unreachable.quality(probes[0][1], target)
    finest = ask(0)
    if not finest >= target:
        raise Unreachable.quality(finest, target)
    lo, hi = 0, L - 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if ask(mid) >= target:
            lo = mid
        else:
            hi = mid
    return lo, probes
