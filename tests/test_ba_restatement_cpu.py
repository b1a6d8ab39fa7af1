"""tests/ba_restatement.py (the fp64 Gauss-Newton step derived from the residual by autograd) against the fp32 CPU
oracle, and the GPU test's metric against deliberately wrong steps.  No GPU.

Anchor: on every problem of the GPU test the derived step and `oracle.droid_oracle.ba` (the reference's hand-written
Jacobians, restated in fp32) agree to 1e-4 of the largest entry of dx and of dz at both damping levels -- the tolerance
tests/test_track_gpu.py already applies between two fp32 implementations of this step; a difference in the derivation
(a sign, an adjoint, the depth prior, the back-substitution quirk) is of order 1e-2 .. 1, see the sensitivity test.
(Run in fp64 with an fp64 pixel grid, the oracle's formulas agree with the autograd Jacobians to 5e-14 per element.)

Sensitivity: err() of ba_restatement applied to four subtly wrong steps exceeds bound(err_oracle32) -- what the GPU test
allows a kernel -- at least ten times (measured: 2e3 .. 2e5 times).  The three that change the assembled system do so at
both damping levels; `evt_quirk=False` changes only the E^T dx term of the back-substitution, which the probe's damping
(dx ~ b / ep ~ 1e-6) takes down with dx, so it is required at production damping, which every GPU case runs as well."""
import inspect
import textwrap

import pytest
import torch

import ba_restatement as R
from oracle import droid_oracle as O

DAMPINGS = ("production", "probe")


def _oracle(prob, motion_only, iters, lm, ep, **kw):
    po, do = prob["poses"].clone(), prob["disps"].clone()
    dx, dz = O.ba(po, do, prob["intrinsics"], prob["disps_sens"], prob["target"], prob["weight"], prob["eta"],
                  prob["ii"], prob["jj"], prob["t0"], prob["t1"], iters, lm, ep, motion_only, **kw)
    return dx, dz, po, do


@pytest.mark.parametrize("name", R.CASES)
def test_inputs_keep_clear_of_the_depth_mask_and_exercise_it(name):
    R.check_inputs(R.reference(name, "production")[0]["z"])


@pytest.mark.parametrize("damping", DAMPINGS)
@pytest.mark.parametrize("name", R.CASES)
def test_anchor_derived_step_is_the_oracles_step(name, damping):
    prob, motion_only, iters = R.case(name)
    ref, lm, ep = R.reference(name, damping)
    dx, dz, po, do = _oracle(prob, motion_only, iters, lm, ep)
    print(f"{name} {damping}: ep {ep:.4g} err_oracle32 dx {R.err(dx, ref['dx']):.2e}"
          + ("" if motion_only else f" dz {R.err(dz, ref['dz']):.2e}"))
    if damping == "probe":                       # the probe is what it says: condition number ~1
        assert float(torch.linalg.cond(ref["H"])) < 1.01
    assert R.err(dx, ref["dx"]) < 1e-4
    torch.testing.assert_close(po.double(), ref["poses"], rtol=0, atol=1e-5)
    if motion_only:
        assert dz is None and ref["dz"] is None and torch.equal(ref["disps"], prob["disps"].double())
    else:
        assert R.err(dz, ref["dz"]) < 1e-4
        torch.testing.assert_close(do.double(), ref["disps"], rtol=0, atol=1e-5)


def test_zero_weight_edges_leave_the_step_unchanged():
    """"short-lists-padded" is compared with the fp64 step of "short-lists": the restatement gives the same for both."""
    ref, lm, ep = R.reference("short-lists", "production")
    pad = R.ba(R.case("short-lists-padded")[0], 1, lm, ep)
    assert len(pad["z"][0]) == 54 and len(ref["z"][0]) == 30
    torch.testing.assert_close(pad["dx"], ref["dx"], rtol=1e-12, atol=0)
    torch.testing.assert_close(pad["dz"], ref["dz"], rtol=1e-12, atol=1e-18)


def test_graphs_reach_the_structural_edges():
    prob = R.case("long-lists")[0]
    ii, jj, t0, t1 = prob["ii"], prob["jj"], prob["t0"], prob["t1"]
    M = prob["eta"].shape[0]
    deg = torch.bincount(ii, minlength=12)
    assert len(ii) >= 6 * M and M == 9
    assert set([1, 2, 3, 5, 9]) <= set(deg.tolist()) and int(deg[9]) == 0 and t0 <= 9 < t1
    assert bool((ii == jj).any()) and bool((ii < t0).any()) and bool(((jj < t0) | (jj >= t1)).any())
    short = R.case("short-lists")[0]
    assert len(short["ii"]) < 6 * M and short["eta"].shape[0] == M and torch.equal(short["poses"], prob["poses"])
    assert len(R.case("short-lists-padded")[0]["ii"]) >= 6 * M
    big = R.case("1030-frames")[0]
    assert big["poses"].shape[0] == 1030 > 1024 and (big["t0"], big["t1"]) == (1000, 1012)
    src = set(big["ii"].tolist())
    assert {3, 4, 5, 517, 1029} <= src and min(src) < 1000 < 1029 == max(src)


def test_retraction_is_the_group_exponential():
    """retract() (the reference's branches) against the matrix exponential: equal above theta = 1e-4, below it short of
    the translation's rotational terms only (< theta |tau|); the poses are those of a test problem."""
    g = torch.Generator().manual_seed(5)
    poses = R.case("5x7-mix")[0]["poses"][:4]
    for theta in (1e-6, 5e-5, 1e-3, 0.3):
        xi = torch.randn(4, 6, generator=g, dtype=torch.float64)
        xi[:, 3:] *= theta / xi[:, 3:].norm(dim=-1, keepdim=True)
        out = R.pose_matrix(R.retract(xi, poses))
        exact = torch.stack([R._exp(x) for x in xi]) @ R.pose_matrix(poses)
        tol = 1e-12 + 1.2e-7 * theta              # (the fp32 quaternions' defect | |q|^2 - 1 | times the angle)
        if theta <= 1e-4:
            tol += theta * float(xi[:, :3].norm(dim=-1).max())
        assert float((out - exact).abs().max()) < tol


@pytest.mark.parametrize("theta", R.SMALL_ANGLE_TARGETS)
def test_small_angle_cases_lie_on_the_intended_side_of_both_thresholds(theta):
    prob, ref = R.small_angle_case(theta)
    R.check_inputs(ref["z"])
    th = ref["dx"][:, 3:].norm(dim=-1)
    print(f"theta {theta:g}: rotation norms of the fp64 dx {[f'{t:.2e}' for t in th.tolist()]}")
    assert 0.9 * theta < float(th.max()) < 1.1 * theta
    if theta < 1e-4:       # Taylor quaternion (theta^2 < 1e-8), translation without its rotational terms
        assert bool((th * th < 0.5e-8).all()) and bool((th < 0.7e-4).all())
    else:                  # sinf / cosf quaternion and the rotational terms of the translation, for most of the window
        assert int((th > 2e-4).sum()) >= 4 and bool((th * th > 4e-8)[th > 2e-4].all())


# -------------------------------------------------------------------------------------------------- sensitivity ----
def _rewritten(fn, old, new, count):
    """`fn` recompiled in its own module's namespace with `old` replaced by `new` (exactly `count` times)."""
    src = textwrap.dedent(inspect.getsource(fn))
    assert src.count(old) == count, (fn.__name__, old, src.count(old))
    scope = {}
    exec(compile(src.replace(old, new), f"<{fn.__name__}: {old} -> {new}>", "exec"), fn.__globals__, scope)
    return scope[fn.__name__]


def _flip_ji_of_edge(e):
    adj = O.se3.adj_se3

    def flipped(t, q, X):
        out = adj(t, q, X).clone()
        out[e] = -out[e]
        return out
    return flipped


@pytest.mark.parametrize("damping", DAMPINGS)
@pytest.mark.parametrize("name", ["5x7-mix", "long-lists"])
def test_metric_rejects_subtly_wrong_steps(name, damping, monkeypatch):
    prob, motion_only, iters = R.case(name)
    ref, lm, ep = R.reference(name, damping)
    dx, dz, _, _ = _oracle(prob, motion_only, iters, lm, ep)
    bound_dx, bound_dz = R.bound(R.err(dx, ref["dx"])), R.bound(R.err(dz, ref["dz"]))
    e = next(n for n in range(len(prob["ii"])) if prob["t0"] <= int(prob["ii"][n]) < prob["t1"]
             and prob["t0"] <= int(prob["jj"][n]) < prob["t1"] and int(prob["ii"][n]) != int(prob["jj"][n]))

    def excess(**kw):
        mx, mz, _, _ = _oracle(prob, motion_only, iters, lm, ep, **kw)
        return max(R.err(mx, ref["dx"]) / bound_dx, R.err(mz, ref["dz"]) / bound_dz)

    found = {"evt_quirk=False": excess(evt_quirk=False)}
    with monkeypatch.context() as mp:
        mp.setattr(O, "ba", _rewritten(O.ba, "alpha = 0.05", "alpha = 0.06", 1))
        found["alpha 0.06"] = excess()
    with monkeypatch.context() as mp:
        mp.setattr(O, "ba_edge_terms", _rewritten(O.ba_edge_terms, "0.001 * wt", "0.0011 * wt", 2))
        found["weight scale 0.0011"] = excess()
    with monkeypatch.context() as mp:
        mp.setattr(O.se3, "adj_se3", _flip_ji_of_edge(e))
        found[f"-Ji of edge {e}"] = excess()
    print(f"{name} {damping}: bound dx {bound_dx:.2e} dz {bound_dz:.2e}; err / bound of the wrong steps: "
          + ", ".join(f"{k} {v:.3g}" for k, v in found.items()))
    assert excess() <= 0.25 + 1e-12, "the patches are undone: the oracle itself sits at bound / 4 or below"
    for k, v in found.items():
        if damping == "probe" and k.startswith("evt_quirk"):
            continue        # (see the module docstring: the probe takes dx, and with it this term of dz, down to ~1e-6)
        assert v >= 10.0, f"{k}: err / bound = {v:.3g}"
