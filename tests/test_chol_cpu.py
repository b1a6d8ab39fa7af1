"""The fp64 Cholesky restatement (tests/chol_restatement.py) against numpy, the exact-failure constructions the GPU tests
rely on, and gs_chol_solve's refusal of bad arguments -- all without a GPU."""
import ctypes

import numpy as np
import pytest

import chol_restatement as R


@pytest.mark.parametrize("n", [1, 6, 31, 64, 150])
@pytest.mark.parametrize("lm,ep", [(1e-4, 0.1), (0.0, 0.0)])
def test_restatement_matches_numpy_on_spd(n, lm, ep):
    rng = np.random.default_rng(n)
    A = R.spd(n, 1e3, rng)
    b = rng.standard_normal(n)
    S = R.damp(A, lm, ep)
    L, k = R.cholesky(S)
    assert k is None
    np.testing.assert_allclose(L, np.linalg.cholesky(S), rtol=0, atol=1e-12 * np.abs(L).max())
    x = R.substitute(L, b)
    np.testing.assert_allclose(x, np.linalg.solve(S, b), rtol=1e-9, atol=1e-9 * np.abs(x).max())
    dx, fail = R.restate(A, b, lm, ep)
    assert fail is None and np.array_equal(dx, x.astype(np.float32))


def test_damping_rounds_lm_ep_to_float32_and_reads_the_lower_triangle():
    rng = np.random.default_rng(3)
    A = R.spd(12, 10.0, rng)
    B = A.copy()
    B[np.triu_indices(12, 1)] = np.nan
    S = R.damp(B, 1e-4, 0.1)
    assert np.array_equal(S, S.T) and not np.isnan(S).any()
    d = np.diag(A)
    lm, ep = float(np.float32(1e-4)), float(np.float32(0.1))
    assert lm != 1e-4 and ep != 0.1
    assert np.array_equal(np.diag(S), d + (ep + lm * d))
    off = ~np.eye(12, dtype=bool)
    assert np.array_equal(S[off], np.tril(A)[off] + np.tril(A, -1).T[off])


def test_restatement_nan_pivot_is_not_a_failure():
    rng = np.random.default_rng(4)
    A = R.spd(18, 10.0, rng)
    A[7, 3] = np.nan
    dx, k = R.restate(A, rng.standard_normal(18), 0.0, 0.0)
    assert k is None and np.isnan(dx).all()


@pytest.mark.parametrize("n,k", [(6, 0), (6, 5), (150, 59), (150, 149), (200, 64), (200, 199), (294, 120)])
@pytest.mark.parametrize("delta", [1, 0])
def test_exact_failure_fails_at_column_k_only(n, k, delta):
    rng = np.random.default_rng(n * 1000 + k)
    A = R.exact_failure(n, k, delta, rng)
    assert np.abs(A).max() < 2.0 ** 53 and np.array_equal(A, np.round(A))
    S = R.damp(A, 0.0, 0.0)
    assert np.array_equal(S, np.tril(A) + np.tril(A, -1).T)
    L, kf = R.cholesky(S)
    assert kf == k
    assert np.array_equal(np.diag(L)[:k], np.ones(k))          # every earlier pivot is exactly 1
    assert np.array_equal(L[:, :k], np.round(L[:, :k]))        # ... and every earlier column an integer one
    # the pivot reached at column k is exactly -delta
    assert S[k, k] - np.sum(L[k, :k] ** 2) == -delta
    dx, kr = R.restate(A, np.ones(n), 0.0, 0.0)
    assert kr == k and not dx.any()


@pytest.mark.parametrize("n,kappa", [(6, 1e2), (150, 1e6), (294, 1e10), (600, 1e10)])
def test_refined_reference_residual(n, kappa):
    """|b - S x_ref| (long double) within n u (|S| |x_ref| + |b|), componentwise"""
    rng = np.random.default_rng(n)
    S = R.damp(R.spd(n, kappa, rng), 0.0, 0.0)
    b = rng.standard_normal(n)
    x = R.reference_solution(S, b)
    r = np.abs(R.residual_longdouble(S, x, b)).astype(np.float64)
    bound = n * R.U * (np.abs(S) @ np.abs(x) + np.abs(b))
    assert (r <= bound).all(), float((r / bound).max())


def test_scaled_condition_is_scaling_invariant():
    rng = np.random.default_rng(5)
    A = R.spd(60, 1e4, rng)
    D = R.scaled(A, rng)
    k0, _ = R.scaled_condition(A)
    k1, _ = R.scaled_condition(D)
    assert abs(k1 / k0 - 1) < 1e-6
    assert np.linalg.cond(D) > 1e6 * k1


def test_midpoint_distance():
    f = np.float32(1.5)
    up = float(np.nextafter(f, np.float32(2)))
    mid = 0.5 * (1.5 + up)
    assert R.midpoint_distance(np.array([mid]))[0] == 0.0
    assert R.midpoint_distance(np.array([1.5]))[0] == pytest.approx(0.5 * (up - 1.5))


# ---- gs_chol_solve's argument checks: refused before any HIP call (NULL buffers; nothing is enqueued) -------------
GS_ERR_INVALID_ARG, GS_ERR_UNSUPPORTED = -1, -4


def _accepts(n, path):
    if path == 0 or path == 3:
        return n >= 1
    if path == 1:
        return 1 <= n <= 192 and n % 6 == 0
    if path == 2:
        return 1 <= n <= 300 and n % 6 == 0
    return False


def test_chol_solve_refuses_bad_arguments_without_a_gpu(built_lib):
    from go_slam_amd import _lib
    L = _lib.lib()
    null = ctypes.c_void_p(0)
    checked = 0
    for n in [-6, -1, 0] + list(range(1, 461)) + [594, 600, 1194, 1200, 1206]:
        for path in [-1, 0, 1, 2, 3, 4, 7]:
            rc = L.gs_chol_solve(null, null, n, 1e-4, 0.1, path, null, null, null)
            msg = L.gs_last_error().decode()
            if n < 1 or path not in (0, 1, 2, 3):
                assert rc == GS_ERR_INVALID_ARG, (n, path, rc)
            elif not _accepts(n, path):
                assert rc == GS_ERR_UNSUPPORTED, (n, path, rc)
                assert ("small" if path == 1 else "mid") in msg, msg
            else:
                # an accepted (n, path): the only thing wrong is the NULL buffers, still refused before any launch
                assert rc == GS_ERR_INVALID_ARG and "null" in msg, (n, path, rc, msg)
            checked += 1
    assert checked == 7 * 468
