"""Regenerate the signed-sample golden fixtures (``signed_*.npz``) from the specification.

    python tests/golden/make_golden_signed.py

Inputs and expected outputs only (data).  The outputs come from ``tests/signed_spec.py``: the
oracle's mean-predictor codec on ``M(x) = x ^ signbit``, lowres mapped back to the signed type."""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, '..', '..')))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, '..')))

import signed_spec as S  # noqa: E402

CASES = (('signed_vol_i16', (2, 11, 12, 16, 1), np.int16, 3), ('signed_img_i8', (2, 17, 32, 1), np.int8, 2))


def main():
    for name, shape, dtype, ndim in CASES:
        x = S.data(shape, dtype, seed=5)
        for p in (0, 1):
            fn = S.mean_fn(p, ndim)
            lo, maps, dims = S.encode(x, fn, ndim, p)
            assert np.array_equal(S.decode(lo, maps, dims, fn, ndim, p), x), name
            out = {'highres': x, 'lowres': lo, 'dims': np.array(dims, np.int32), 'padding': np.int32(p),
                   'ndim': np.int32(ndim)}
            for i, m in enumerate(maps):
                out[f'map{i}'] = m
            np.savez_compressed(os.path.join(HERE, f'{name}_p{p}.npz'), **out)
            print(name, p, x.shape, x.dtype, 'dims', dims)


if __name__ == '__main__':
    main()
