"""gs_chol_solve (go_slam_amd/csrc/chol.hip) on every path against the fp64 restatement in tests/chol_restatement.py.

The solver is Eigen's SimplicialLLT on S = A + diag(ep + lm diag(A)) (lm, ep rounded to float32 first), dx = float32(x).
u = 2^-53.  S is built from A's lower triangle exactly as the kernels build it, so every check below compares the
kernels with the same fp64 matrix.

Bounds.
  * Reference: x_ref = numpy.linalg.solve(S, b) plus one refinement step with the residual in long double; its error is
    far below every allowance here (tests/test_chol_cpu.py bounds its residual by n u (|S||x| + |b|)).
  * Forward error allowance of an fp64 Cholesky solve, per component:
        E_i = c n u kappa ||x_ref / d||_inf d_i,   d = diag(S)^-1/2,  kappa = cond_2(d S d),  c = 4.
    Cholesky solves (S + dS) x = b with |dS| <= gamma_{3n+1} |L||L^T| (Higham, Thm 10.4), and it is invariant under the
    diagonal scaling d (van der Sluis), so the error is governed by the equilibrated matrix: c = 3 is gamma_{3n+1} / (n u)
    and the remaining 1 covers ||(|L||L^T|)|| / ||S|| > 1 and the norm changes.  For an evenly weighted matrix this is
    c n u kappa ||x_ref||_inf; for the D A D matrices it keeps its meaning where cond_2(S) itself reaches 1e12 and more.
  * Sharp check (kappa <= 1e2, every n up to 1206): E is then below ~1e-10 ||x||, so dx must be bit-equal to
    float32(x_ref).  The only exceptions allowed are components whose x_ref lies within E_i (+ 4 u |x_ref|) of a float32
    rounding midpoint; they may be 1 ulp off.  They are computed one by one, no percentage is allowed.
  * Every solve: |dx - x_ref| <= 0.5 ulp32(|x_ref| + E) + E.
  * Blocked path, its in-place results checked in fp64 (L in H's lower triangle), independent of conditioning:
        |L L^T - S| <= (2n + 8) u |L||L^T|,     |L y - b| <= (2n + 8) u |L||y|
    (gamma_{n+1} of the factorisation / substitution, two roundings of the pivot's reciprocal square root, and gamma_n of
    the check's own fp64 product; (2n + 8) <= 10 n).  y = L^-1 b is in b only where the backward substitution has not
    reused b for its partial sums: for n <= 128 (one 64- or 128-row launch); y is checked there.
  * Square roots: a diagonal S with pivots 2^-900 .. 2^900 (lm = ep = 0): L[j][j] within 1 fp64 ulp of the correctly
    rounded sqrt, off-diagonal L exactly 0.  dx leaves the float32 range there and is not checked.  Subnormal pivots
    are out of scope.
Failure: the exact-failure matrices (tests/chol_restatement.py: exact_failure) reach a pivot of exactly -1 or 0 at
column k with every earlier pivot exactly 1.  dx = 0 everywhere, status[0] = 1, status[1] grows by exactly 1; a good
solve on the same status clears status[0] and leaves status[1].  NaN: no failure, NaN pattern equal to the
restatement's.  Only the lower triangle is read: NaN or 1e300 in the strict upper triangle leave dx bit-equal.  Two
solves of one input are bit-equal (dx, and L on the blocked path).

Paths (gs_chol_solve's `path`): 0 = the product's choice, 1 = small (n <= 192, n % 6 == 0), 2 = mid (n <= 300,
n % 6 == 0), 3 = blocked (any n).  Every solve gets fresh device copies of H and b: the mid and blocked paths work in
place.  The worst error-to-bound ratio of each path (for dx: the error beyond float32(x_ref)'s own rounding, over E)
is written to $CHOL_NUMERICS_REPORT (JSON) when it is set."""
import json
import os

import numpy as np
import pytest
import torch

import chol_restatement as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
C_FWD = 4.0
DAMPING = [(1e-4, 0.1), (1e-5, 1e-2), (0.0, 0.0)]
SWEEP = list(range(6, 457, 6)) + [594, 600, 1194, 1200, 1206]
BLOCKED_N = list(range(1, 201)) + list(range(204, 457, 6))
PATH_NAME = {0: "dispatch", 1: "small", 2: "mid", 3: "blocked"}

_stats = {"solves": 0, "ratio": {}, "midpoint_exceptions": 0}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    out = os.environ.get("CHOL_NUMERICS_REPORT")
    if out:
        with open(out, "w") as f:
            json.dump(_stats, f, indent=1, sort_keys=True)


def _note(key, ratio):
    _stats["ratio"][key] = max(_stats["ratio"].get(key, 0.0), float(ratio))


def accepts(n, path):
    if path in (0, 3):
        return n >= 1
    if path == 1:
        return n <= 192 and n % 6 == 0
    return n <= 300 and n % 6 == 0


def solve(A, b, lm, ep, path, status=None):
    """(dx, status, H after, b after); dx starts as NaN so that every element must be written"""
    from go_slam_amd import _lib
    n = len(b)
    H = torch.tensor(np.ascontiguousarray(A, np.float64), device=DEV)
    bv = torch.tensor(np.ascontiguousarray(b, np.float64), device=DEV)
    dx = torch.full((n,), float("nan"), dtype=torch.float32, device=DEV)
    st = torch.zeros(4, dtype=torch.int32, device=DEV) if status is None else status
    _lib.check(_lib.lib().gs_chol_solve(_lib.ptr(H), _lib.ptr(bv), n, lm, ep, path, _lib.ptr(dx), _lib.ptr(st),
                                        _lib.stream_ptr(DEV)), "gs_chol_solve")
    torch.cuda.synchronize()
    _stats["solves"] += 1
    return dx.cpu().numpy(), st, H.cpu().numpy(), bv.cpu().numpy()


def check_solution(dx, S, b, what, key, sharp=None):
    """dx against x_ref within the forward bound; bit-equal to float32(x_ref) up to the midpoint exceptions when the
    equilibrated condition number is <= 1e2 (or `sharp` says so)"""
    x = R.reference_solution(S, b)
    E, kappa = R.forward_bound(S, x, C_FWD)
    assert not np.isnan(dx).any(), f"{what}: NaN in dx"
    err = np.abs(dx.astype(np.float64) - x)
    allow = 0.5 * R.ulp32(np.abs(x) + E) + E
    bad = err > allow
    if bad.any():
        i = np.flatnonzero(bad)[:6]
        raise AssertionError(f"{what}: {int(bad.sum())} of {len(x)} beyond the bound (kappa {kappa:.3g}) at {i}: "
                             f"dx {dx[i]} x_ref {x[i]} err {err[i]} allow {allow[i]}")
    # reported: the error beyond float32(x_ref)'s own rounding, over the fp64 allowance E (0 where dx is bit-equal)
    _note(key, (np.maximum(err - np.abs(x.astype(np.float32).astype(np.float64) - x), 0.0) / E).max())
    if sharp is None:
        sharp = kappa <= 1e2
    if sharp:
        d = R.ulps32(dx, x.astype(np.float32))
        near = R.midpoint_distance(x) <= E + 4 * R.U * np.abs(x)
        ok = (d == 0) | (near & (d <= 1))
        if not ok.all():
            i = np.flatnonzero(~ok)[:6]
            raise AssertionError(f"{what}: {int((~ok).sum())} components not float32(x_ref) (kappa {kappa:.3g}) at "
                                 f"{i}: dx {dx[i]} x_ref {x[i]} ulps {d[i]}")
        _stats["midpoint_exceptions"] += int((d != 0).sum())
    return x


def check_blocked_in_place(H, bout, S, b, what):
    """L L^T = S and (n <= 128) L y = b, backward errors in fp64"""
    n = len(b)
    L = np.tril(H)
    r = np.abs(L @ L.T - S)
    bound = R.factor_backward_bound(L)
    assert (r <= bound).all(), f"{what}: |L L^T - S| / bound = {float((r / bound).max()):.3g}"
    _note("blocked/LLT_backward", (r / bound).max())
    if n <= 128:
        ry = np.abs(L @ bout - b)
        by = R.substitution_backward_bound(L, bout)
        assert (ry <= by).all(), f"{what}: |L y - b| / bound = {float((ry / by).max()):.3g}"
        _note("blocked/Ly_backward", (ry / by).max())


def status_of(st):
    return [int(v) for v in st.cpu().tolist()[:2]]


# ---------------------------------------------------------------------------------------- product dispatch ----
def _families(n, rng):
    fam = {"kappa1e2": R.spd(n, 1e2, rng), "kappa1e10": R.spd(n, 1e10, rng), "DAD": R.scaled(R.spd(n, 1e2, rng), rng)}
    fam["arrowhead"] = R.block_arrowhead(n, rng)
    return fam


@pytest.mark.parametrize("n", SWEEP)
def test_dispatch_size_sweep(n):
    rng = np.random.default_rng(10_000 + n)
    b = rng.standard_normal(n)
    for name, A in _families(n, rng).items():
        for lm, ep in DAMPING:
            S = R.damp(A, lm, ep)
            dx, st, _, _ = solve(A, b, lm, ep, 0)
            assert status_of(st) == [0, 0], (n, name, lm, ep, status_of(st))
            check_solution(dx, S, b, f"n={n} {name} lm={lm} ep={ep}", "dispatch")


# ---------------------------------------------------------------------------------------------- forced paths ----
@pytest.mark.parametrize("n", BLOCKED_N)
def test_blocked_path_every_edge(n):
    """n < 32, 32, 33, 64 = SB, 65, 128, 129, odd and even numbers of substitution blocks, single-column last panels"""
    rng = np.random.default_rng(20_000 + n)
    A = R.spd(n, 1e2, rng)
    b = rng.standard_normal(n)
    lm, ep = DAMPING[n % 3]
    S = R.damp(A, lm, ep)
    dx, st, H, bout = solve(A, b, lm, ep, 3)
    assert status_of(st) == [0, 0]
    check_solution(dx, S, b, f"blocked n={n}", "blocked")
    check_blocked_in_place(H, bout, S, b, f"blocked n={n}")


@pytest.mark.parametrize("n", [1, 31, 33, 64, 65, 129, 200, 294, 456, 1194])
def test_blocked_in_place_ill_conditioned(n):
    """the backward-error checks do not depend on conditioning: kappa = 1e10 and D A D"""
    rng = np.random.default_rng(25_000 + n)
    b = rng.standard_normal(n)
    for name, A in {"kappa1e10": R.spd(n, 1e10, rng), "DAD": R.scaled(R.spd(n, 1e4, rng), rng)}.items():
        S = R.damp(A, 0.0, 0.0)
        dx, st, H, bout = solve(A, b, 0.0, 0.0, 3)
        assert status_of(st) == [0, 0]
        check_solution(dx, S, b, f"blocked n={n} {name}", "blocked")
        check_blocked_in_place(H, bout, S, b, f"blocked n={n} {name}")


@pytest.mark.parametrize("n", list(range(6, 301, 6)))
def test_small_and_mid_every_n_and_cross_path(n):
    """every n the small and mid paths accept, the same matrix through every accepted path (and the dispatch)"""
    rng = np.random.default_rng(30_000 + n)
    b = rng.standard_normal(n)
    for name, A in {"kappa1e2": R.spd(n, 1e2, rng), "kappa1e8": R.spd(n, 1e8, rng)}.items():
        lm, ep = DAMPING[(n // 6) % 3]
        S = R.damp(A, lm, ep)
        got = {}
        for path in (0, 1, 2, 3):
            if not accepts(n, path):
                continue
            dx, st, _, _ = solve(A, b, lm, ep, path)
            assert status_of(st) == [0, 0], (n, path)
            check_solution(dx, S, b, f"{PATH_NAME[path]} n={n} {name}", PATH_NAME[path])
            got[path] = dx
        assert set(got) == ({0, 1, 2, 3} if n <= 192 else {0, 2, 3})
        assert np.array_equal(got[0], got[1 if n <= 192 else 2]), f"n={n}: the dispatch is not the path it names"


def test_blocked_pivot_square_roots():
    """diagonal S, pivots 2^-900 .. 2^900: L[j][j] within 1 ulp of the correctly rounded square root"""
    rng = np.random.default_rng(5)
    for n in (181, 200):
        e = np.round(np.linspace(-900, 900, n)).astype(int)
        p = np.ldexp(rng.uniform(1.0, 2.0, n), e)
        A = np.diag(p)
        _, st, H, _ = solve(A, rng.standard_normal(n), 0.0, 0.0, 3)
        assert status_of(st) == [0, 0]
        d = np.diag(H)
        ref = np.sqrt(p)
        ulp = np.abs(d.view(np.int64) - ref.view(np.int64))
        assert ulp.max() <= 1, (n, int(ulp.max()), e[np.argmax(ulp)])
        assert not np.tril(H, -1).any()


# --------------------------------------------------------------------------------------------------- failure ----
FAIL_CASES = ([(150, k, p) for k in (0, 5, 11, 29, 30, 64, 80, 95, 149) for p in (0, 1, 2, 3)]
              + [(294, k, p) for k in (0, 5, 29, 30, 59, 60, 64, 80, 95, 119, 120, 250, 293) for p in (0, 2, 3)]
              + [(200, k, 3) for k in (0, 5, 64, 80, 95, 192, 199)]
              + [(1194, k, 0) for k in (0, 59, 60, 64, 95, 600, 1183, 1184, 1193)])


@pytest.mark.parametrize("n,k,path", FAIL_CASES)
def test_failure_at_column_k(n, k, path):
    rng = np.random.default_rng(40_000 + 7 * n + k)
    b = rng.standard_normal(n)
    good = R.spd(n, 1e2, rng)
    st = torch.tensor([0, 5, 0, 0], dtype=torch.int32, device=DEV)
    count = 5
    for delta in (1, 0):
        A = R.exact_failure(n, k, delta, rng)
        if n <= 300:
            assert R.cholesky(R.damp(A, 0.0, 0.0))[1] == k
        dx, st, _, _ = solve(A, b, 0.0, 0.0, path, st)
        count += 1
        assert status_of(st) == [1, count], (n, k, path, delta, status_of(st))
        assert np.array_equal(dx, np.zeros(n, np.float32)), (n, k, path, delta, np.flatnonzero(dx != 0)[:8])
        dx, st, _, _ = solve(good, b, 1e-4, 0.1, path, st)
        assert status_of(st) == [0, count], (n, k, path, delta, status_of(st))
        check_solution(dx, R.damp(good, 1e-4, 0.1), b, f"after failure n={n} k={k}", PATH_NAME[path])


# ------------------------------------------------------------------------- NaN, lower triangle, reproducibility ----
CASES = [(150, 0), (150, 1), (150, 2), (150, 3), (294, 0), (294, 2), (294, 3), (200, 3), (33, 3), (1194, 0)]


@pytest.mark.parametrize("n,path", CASES)
def test_nan_propagates_without_failure(n, path):
    rng = np.random.default_rng(50_000 + n)
    A = R.spd(n, 1e2, rng)
    b = rng.standard_normal(n)
    i, j = n - 1 - n // 3, n // 4
    variants = {"offdiag": (A, b, (i, j)), "diag": (A, b, (n // 2, n // 2)), "b": (A, b, None)}
    for name, (A0, b0, at) in variants.items():
        A1, b1 = A0.copy(), b0.copy()
        if at is None:
            b1[n // 3] = np.nan
        else:
            A1[at] = np.nan
        ref, k = R.restate(A1, b1, 1e-4, 0.1)
        assert k is None
        st = torch.tensor([0, 3, 0, 0], dtype=torch.int32, device=DEV)
        dx, st, _, _ = solve(A1, b1, 1e-4, 0.1, path, st)
        assert status_of(st) == [0, 3], (n, path, name, status_of(st))
        assert np.array_equal(np.isnan(dx), np.isnan(ref)), (n, path, name, int(np.isnan(dx).sum()),
                                                             int(np.isnan(ref).sum()))


@pytest.mark.parametrize("n,path", CASES)
def test_only_the_lower_triangle_is_read(n, path):
    rng = np.random.default_rng(60_000 + n)
    A = R.spd(n, 1e2, rng)
    b = rng.standard_normal(n)
    dx0, _, _, _ = solve(A, b, 1e-4, 0.1, path)
    up = np.triu_indices(n, 1)
    for fill in (np.nan, 1e300):
        A1 = A.copy()
        A1[up] = fill
        dx1, st, _, _ = solve(A1, b, 1e-4, 0.1, path)
        assert status_of(st) == [0, 0]
        assert np.array_equal(dx1.view(np.int32), dx0.view(np.int32)), (n, path, fill)


@pytest.mark.parametrize("n,path", CASES + [(456, 3), (1206, 0)])
def test_bitwise_reproducible(n, path):
    rng = np.random.default_rng(70_000 + n)
    A = R.spd(n, 1e6, rng)
    b = rng.standard_normal(n)
    dx0, _, H0, _ = solve(A, b, 1e-5, 1e-2, path)
    dx1, _, H1, _ = solve(A, b, 1e-5, 1e-2, path)
    assert np.array_equal(dx0.view(np.int32), dx1.view(np.int32))
    if path == 3 or (path == 0 and n > 300):
        assert np.array_equal(np.tril(H0).view(np.int64), np.tril(H1).view(np.int64))
