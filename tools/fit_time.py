"""Time the fused moment kernel (kmp_linear_moments, kmp_fit.hip) at C3 geometry against the
composition of primitives that computes the same matrix without it: kmp_pad (reflect, then
symmetric), kmp_lowres_from_highres, kmp_features_from_lowres, kmp_targets_from_highres, a torch
cast to float64 and ``X.T @ X``.  HIP events, median of ``reps`` after warm-up.  ``X.T @ X`` of a
[16.8 M, Q] matrix is one output tile with no split along the cells, so the composition is also timed
with the product taken per tile (``bmm`` over [tiles, 32768, Q], then a sum): the fairer baseline.

    python tools/fit_time.py [tiles=512] [reps=20]
"""
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kompressor_amd as kom  # noqa: E402
from kompressor_amd import _device as dev, _lib, _nd  # noqa: E402
from kompressor_amd._lib import check, lib  # noqa: E402

COPY_CEILING = 6.3e12  # bytes/s, the measured copy ceiling the other rows are quoted against


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms)


def design(h, p):
    hp, _ = _nd.d_pad_highres(h, 3)
    lo = _nd.d_lowres_from_highres(hp, 3)
    F = _nd.d_features_from_lowres(_nd.d_pad_neighborhood(lo, p, 3), p, 3)
    T = _nd.d_targets_from_highres(hp, 3)
    n = F.shape[-2]
    # torch's uint16 support is thin: widen through the int16 view (part of the composition's cost)
    def f64(t):
        return t.view(torch.int16).to(torch.int32).bitwise_and_(0xFFFF).to(torch.float64)

    return torch.cat([f64(F.reshape(-1, n)), f64(T.reshape(-1, 19)),
                      torch.ones((F.numel() // n, 1), dtype=torch.float64, device=h.device)], dim=1)


def composition(h, p, per_tile=False):
    X = design(h, p)
    if per_tile:
        Xt = X.view(h.shape[0], -1, X.shape[1])
        return torch.bmm(Xt.transpose(1, 2), Xt).sum(0)
    return X.T @ X


def main():
    tiles = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    dev.require_gpu()
    rng = np.random.default_rng(0)
    h = torch.from_numpy(rng.integers(0, 65536, size=(tiles, 64, 64, 64, 1), dtype=np.int64).astype(np.uint16)).cuda()
    cells = tiles * 32 ** 3
    print(f'{_lib.version()}  {tiles} x 64^3 uint16 = {h.numel() * 2 / 1e6:.0f} MB, {cells} cells, median of {reps}')
    for p in (0, 1):
        q = (2 * p + 2) ** 3 + 20
        ws = dev.empty((lib.kmp_linear_moments_workspace_bytes(3, _lib.U16, p) // 8,), torch.int64)
        out = dev.empty((q, q), torch.int64)

        def fused():
            check(lib.kmp_linear_moments(3, _lib.U16, h.data_ptr(), tiles, _lib.i64x3((64, 64, 64)), 1, p,
                                         out.data_ptr(), ws.data_ptr(), dev.stream()), 'linear_moments')

        med, best = timed(fused, reps)
        M = out.cpu().numpy()
        line = f'p={p} fused kmp_linear_moments: median {med:.3f} ms (min {best:.3f}), {med * 1e6 / cells:.4f} ns/cell'
        if p == 0:
            line += f', {h.numel() * 2 / (med * 1e-3) / COPY_CEILING * 100:.1f}% of the 6.3 TB/s copy ceiling on one read'
        print(line)
        # the composition materialises X as float64 (and its uint16 / int32 stages): on a tile subset
        # if that does not fit, scaled per cell
        sub = tiles
        free = torch.cuda.mem_get_info()[0]
        while sub > 1 and sub * 32 ** 3 * q * 8 * 4 > 0.6 * free:
            sub //= 2
        hs = h[:sub]
        note = 'the whole batch' if sub == tiles else f'a subset of {sub} tiles, scaled per cell'
        for per_tile, what in ((False, 'X.T @ X'), (True, 'per-tile bmm + sum')):
            cmed, cbest = timed(lambda: composition(hs, p, per_tile), reps, warmup=2)
            per_cell = cmed * 1e6 / (sub * 32 ** 3)
            print(f'p={p} composition (pad, lowres, features, targets, float64 cast, {what}) on {note}: '
                  f'median {cmed:.3f} ms (min {cbest:.3f}), {per_cell:.4f} ns/cell, '
                  f'{per_cell / (med * 1e6 / cells):.1f}x the fused kernel per cell')
        # the composition's float64 sums pass 2^53 at this size and are inexact; a tile's own products
        # stay below 2^15 * 2^32, so the per-tile float64 matrices are exact and their int64 sum is M
        Ms = kom.linear_moments(hs, p, 3) if sub != tiles else M
        Mc = composition(hs, p).cpu().numpy()
        print(f'p={p} max relative difference fused (exact) vs X.T @ X (float64): '
              f'{np.max(np.abs(Mc - Ms.astype(np.float64)) / np.maximum(1.0, np.abs(Mc))):.2e}')
        Xt = design(hs, p).view(sub, 32 ** 3, q)
        exact = torch.bmm(Xt.transpose(1, 2), Xt).to(torch.int64).sum(0).cpu().numpy()
        print(f'p={p} fused bit-equal to the per-tile float64 products summed in int64: {np.array_equal(exact, Ms)}')


if __name__ == '__main__':
    main()
