"""Host side of the LinearPredictor fit: ``solve_moments`` against numpy's least squares, the
additivity of the moments' specification, and the validation that runs before any device call."""

import numpy as np
import pytest
import torch

import kompressor_amd as kom
from kompressor_amd import predictors as P
from fit_spec import PROBES, PROBE_IDS, PROBE_SEED, design, field, spec_moments


@pytest.mark.parametrize('ndim,shape,dtype,p', PROBES, ids=PROBE_IDS)
def test_solve_moments_matches_lstsq_on_the_design_matrix(ndim, shape, dtype, p):
    """The predictions ``F W + b`` of the centred normal equations agree with ``numpy.linalg.lstsq``
    on the raw float64 design matrix within 1e-4 sample levels (far below the 0.5 level that could
    move a truncated prediction).  Compared before the rounding to the predictor's float32
    parameters (``dtype=float64``): one float32 ulp of a weight times a 16-bit feature is already
    ~4e-3 levels, which says nothing about the solve.  The float32 result is that solution rounded."""
    X, N, K = design(field(shape, PROBE_SEED, dtype), p, ndim)
    M = X.T @ X
    w, b = kom.solve_moments(M, N, round_bias=False, dtype=np.float64)
    A = np.concatenate([X[:, :N], X[:, -1:]], axis=1).astype(np.float64)
    ref = np.linalg.lstsq(A, X[:, N:N + K].astype(np.float64), rcond=None)[0]
    got = X[:, :N].astype(np.float64) @ w + b
    want = X[:, :N].astype(np.float64) @ ref[:N] + ref[N]
    err = np.abs(got - want).max()
    print(f'max |prediction difference| = {err:.3e} sample levels')
    assert err <= 1e-4
    w32, b32 = kom.solve_moments(M, N, round_bias=False)
    assert w32.dtype == np.float32 and b32.dtype == np.float32 and w32.shape == (N, K) and b32.shape == (K,)
    assert np.array_equal(w32, w.astype(np.float32))
    assert (np.abs(b32 - b) <= np.spacing(np.abs(b32))).all()


@pytest.mark.parametrize('ndim,p,c', [(3, 1, 1234), (2, 0, 7)])
def test_constant_input_gives_zero_weights_and_the_constant_plus_half(ndim, p, c):
    h = np.full((2,) + (9,) * ndim + (1,), c, np.uint16)
    M = spec_moments(h, p, ndim)
    w, b = kom.solve_moments(M, (2 * p + 2) ** ndim)
    assert np.array_equal(w, np.zeros_like(w))
    assert np.array_equal(b, np.full_like(b, c + 0.5))


def test_rank_deficient_input_returns_finite_weights():
    # constant along x and y: every feature of one z plane is the same column
    z = np.arange(11, dtype=np.uint16) * 300 + 5
    h = np.broadcast_to(z[None, :, None, None, None], (1, 11, 9, 9, 1)).copy()
    X, N, K = design(h, 1, 3)
    assert np.linalg.matrix_rank(X[:, :N].astype(np.float64)) < N
    w, b = kom.solve_moments(X.T @ X, N, round_bias=False, dtype=np.float64)
    assert np.isfinite(w).all() and np.isfinite(b).all()
    # and it still is a least-squares solution: the fitted values of one are those of any other
    A = np.concatenate([X[:, :N], X[:, -1:]], axis=1).astype(np.float64)
    ref = np.linalg.lstsq(A, X[:, N:N + K].astype(np.float64), rcond=None)[0]
    assert np.abs(X[:, :N] @ w + b - A @ ref).max() <= 1e-4


def test_ridge_shrinks_the_weights():
    ndim, shape, dtype, p = PROBES[1]
    X, N, _ = design(field(shape, PROBE_SEED, dtype), p, ndim)
    M = X.T @ X
    norms = [np.linalg.norm(kom.solve_moments(M, N, ridge=r, dtype=np.float64)[0]) for r in (0.0, 1e-3, 1e-1)]
    assert norms[0] > norms[1] > norms[2] > 0
    with pytest.raises(ValueError):
        kom.solve_moments(M, N, ridge=-1.0)


@pytest.mark.parametrize('ndim,shape,dtype,p', PROBES, ids=PROBE_IDS)
def test_round_bias_is_exactly_one_half(ndim, shape, dtype, p):
    X, N, _ = design(field(shape, PROBE_SEED, dtype), p, ndim)
    M = X.T @ X
    w1, b1 = kom.solve_moments(M, N)
    w0, b0 = kom.solve_moments(M, N, round_bias=False)
    assert np.array_equal(w0, w1)
    assert np.array_equal(b1.astype(np.float64) - b0.astype(np.float64), np.full(b0.shape, 0.5))


@pytest.mark.parametrize('ndim,shape,dtype,p', PROBES, ids=PROBE_IDS)
def test_spec_moments_add_over_the_batch(ndim, shape, dtype, p):
    h = field(shape, PROBE_SEED, dtype)
    whole = spec_moments(h, p, ndim)
    assert np.array_equal(whole, spec_moments(h[:1], p, ndim) + spec_moments(h[1:], p, ndim))
    Q = (2 * p + 2) ** ndim + (19 if ndim == 3 else 5) + 1
    assert whole.shape == (Q, Q) and whole.dtype == np.int64 and np.array_equal(whole, whole.T)
    cells = shape[0] * int(np.prod([s // 2 for s in shape[1:]]))
    assert whole[-1, -1] == cells


def test_solve_moments_rejects_malformed_moments():
    with pytest.raises(ValueError):
        kom.solve_moments(np.zeros((5, 4), np.int64), 2)
    with pytest.raises(ValueError):
        kom.solve_moments(np.zeros((9, 9), np.int64), 8)   # no targets left
    with pytest.raises(ValueError):
        kom.solve_moments(np.zeros((28, 28), np.int64), 8)  # no cells


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to reach the device fails the test."""
    def boom(*a, **k):
        raise RuntimeError('the device was touched')
    monkeypatch.setattr(P.dev, 'to_device', boom)
    monkeypatch.setattr(P.dev, 'require_gpu', boom)
    monkeypatch.setattr(P.dev, 'empty', boom)


@pytest.mark.parametrize('make,padding,ndim,exc', [
    (lambda: np.zeros((1, 9, 9, 9, 1), np.int32), 0, 3, TypeError),          # 32-bit samples
    (lambda: np.zeros((1, 9, 9, 9, 1), np.float32), 0, 3, TypeError),
    (lambda: torch.zeros((1, 9, 9, 1), dtype=torch.int32), 0, 2, TypeError),
    (lambda: np.zeros((1, 9, 9, 9, 2), np.uint8), 0, 3, AssertionError),      # C > 1
    (lambda: np.zeros((1, 9, 9, 9), np.uint8), 0, 3, AssertionError),         # no channel axis
    (lambda: np.zeros((1, 9, 9, 9, 1), np.uint16), 2, 3, AssertionError),     # 3D padding 2
    (lambda: np.zeros((1, 9, 9, 1), np.uint16), 3, 2, AssertionError),        # 2D padding 3
    (lambda: np.zeros((1, 9, 9, 1), np.uint16), -1, 2, AssertionError),
    (lambda: np.zeros((1, 9, 9, 1), np.uint16), 1.0, 2, AssertionError),
    (lambda: np.zeros((1, 9, 9, 1), np.uint16), 0, 4, AssertionError),        # ndim
    (lambda: np.zeros((1, 9, 1, 1), np.uint16), 0, 2, AssertionError),        # a spatial dim below 2
    (lambda: np.zeros((0, 9, 9, 1), np.uint16), 0, 2, AssertionError),        # empty batch
])
def test_unsupported_input_raises_before_any_device_call(no_device, make, padding, ndim, exc):
    with pytest.raises(exc):
        kom.linear_moments(make(), padding, ndim)
    with pytest.raises(exc):
        kom.LinearPredictor.fit(make(), padding, ndim)


def test_too_many_cells_are_rejected_before_any_device_call(no_device):
    # 2^31 cells: a uint16 sum of squares could pass 2^63.  A broadcast view: no memory behind it.
    h = np.broadcast_to(np.zeros((1, 1, 1, 1), np.uint8), (1 << 17, 256, 256, 1))
    with pytest.raises(AssertionError):
        kom.linear_moments(h, 0, 2)


def test_from_moments_builds_the_predictor_without_a_device(no_device):
    ndim, shape, dtype, p = PROBES[4]
    X, N, K = design(field(shape, PROBE_SEED, dtype), p, ndim)
    M = X.T @ X
    pred = kom.LinearPredictor.from_moments(M, p, ndim, arith='f32')
    w, b = kom.solve_moments(M, N)
    assert (pred.padding, pred.ndim, pred.arith) == (p, ndim, 'f32')
    assert np.array_equal(pred.weights.numpy(), w) and np.array_equal(pred.bias.numpy(), b)
    with pytest.raises(ValueError):
        kom.LinearPredictor.fit([], p, ndim)


def test_c_abi_refuses_unsupported_configurations_before_any_launch():
    """kmp_linear_moments returns KMP_ERR_UNSUPPORTED / KMP_ERR_ARG from its argument checks, before
    the first HIP call (the pointers below are never dereferenced)."""
    from kompressor_amd import _lib
    lib, fake = _lib.lib, 0x1000

    def call(nsp, dtype, B, shape, C, p):
        return lib.kmp_linear_moments(nsp, dtype, fake, B, _lib.i64x3(shape), C, p, fake, fake, None)

    assert call(3, _lib.U16, 1, (9, 9, 9), 2, 0) == _lib.KMP_ERR_UNSUPPORTED      # C > 1
    assert call(3, _lib.I32, 1, (9, 9, 9), 1, 0) == _lib.KMP_ERR_UNSUPPORTED      # 32-bit samples
    assert call(3, _lib.F32, 1, (9, 9, 9), 1, 0) == _lib.KMP_ERR_UNSUPPORTED
    assert call(3, _lib.U8, 1, (9, 9, 9), 1, 2) == _lib.KMP_ERR_UNSUPPORTED       # volumes, padding 2
    assert call(2, _lib.U8, 1, (9, 9), 1, 3) == _lib.KMP_ERR_UNSUPPORTED          # images, padding 3
    assert call(2, _lib.U8, 1, (9, 9), 1, -1) == _lib.KMP_ERR_UNSUPPORTED
    assert call(4, _lib.U8, 1, (9, 9, 9), 1, 0) == _lib.KMP_ERR_ARG               # nsp
    assert call(2, _lib.U8, 1 << 17, (256, 256), 1, 0) == _lib.KMP_ERR_ARG        # 2^31 cells
    assert b'2^31' in lib.kmp_last_error()
    assert call(2, _lib.U8, 1, (9, 1), 1, 0) == _lib.KMP_ERR_ARG                  # a spatial dim below 2
    assert lib.kmp_linear_moments(2, _lib.U8, None, 1, _lib.i64x3((9, 9)), 1, 0, fake, fake, None) == _lib.KMP_ERR_ARG
    # 2 (64 + 19) + 1 = 167 byte columns -> 11 blocks of 16
    assert lib.kmp_linear_moments_workspace_bytes(3, _lib.U16, 1) == 176 * 176 * 8
    assert lib.kmp_linear_moments_workspace_bytes(2, _lib.U8, 0) == 16 * 16 * 8
    assert lib.kmp_linear_moments_workspace_bytes(3, _lib.U16, 2) == 0
    assert lib.kmp_linear_moments_workspace_bytes(3, _lib.I32, 0) == 0
