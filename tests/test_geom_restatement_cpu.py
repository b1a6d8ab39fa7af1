"""tests/geom_restatement.py (the fp64 matrix model of reproject, projmap, frame_distance, iproj and depth_filter) against
the fp32 CPU oracle, and the GPU test's checks against deliberately wrong models.  No GPU.

Anchor: on every case of the GPU test, outside the ambiguity band (at most 1 % of a case's results), the oracle's masks,
counts and 1000 branches EQUAL the model's, and its coordinates, points and distances lie within a few fp32 roundings of
the model's (err_oracle32, printed; the GPU test allows a kernel 4 x that figure).

Inputs: each case is shown to contain what it is there for (points below Z = 0.1, between the cut-offs, valid shares,
every count from 0 to 6, exact zero disparities, the frame turned by pi, the negated quaternion, distinct intrinsics).

Sensitivity: each of eleven subtly wrong variants of the model either breaks an exact comparison with the oracle or has
the oracle miss bound(err_oracle32) against it.  Measured (err / bound, or the number of unequal results), the smallest
over the three cases:

    reproject: intrinsics of i and j swapped        err / bound  1.2e+06
    relative pose M_i inv(M_j)                      err / bound  3.2e+06
    reproject valid at 0.25                         unequal      8
    projmap valid at 0.2                            unequal      6
    reproject without the Z < 0.1 substitution      err / bound  8.6e+05
    depth_filter: round for floor                   unequal      72
    depth_filter: u0 <= wd-1                        unequal      12
    depth_filter: neighbours +-1, +-2, +-3          unequal      40
    stereo baseline +0.1                            err / bound  3.2e+04
    frame_distance without the translation leg      err / bound  1.4e+05
    frame_distance: beta and 1 - beta swapped       err / bound  1.7e+05
    frame_distance: <= 0.75                         1000 at exactly 75 % valid (known answer 6.857)

The last one cannot be judged by the oracle.  At a share of exactly 0.75 the oracle returns 1000: it follows the
reference, whose `valid / (total + 1e-8) < 0.75` is evaluated in double (a double literal), so that an exact 0.75 falls
just below.  The kernel evaluates it in fp32, where the 1e-8 vanishes, and returns the distance, which is what
`share < 0.75` says.  The variant is therefore judged by the closed-form answer of frame_distance_kat()."""
import inspect
import math
import textwrap

import pytest
import torch

import geom_restatement as R
from oracle import droid_oracle as O


_ORACLE = {}


def oracle32(name):
    """Every operation of the fp32 oracle on case `name` (computed once)."""
    if name not in _ORACLE:
        _ORACLE[name] = R.run_all(O, R.case(name))
    return _ORACLE[name]


compare = R.compare


@pytest.mark.parametrize("name", R.CASES)
def test_ambiguity_share_is_capped(name):
    shares = R.ambiguity_shares(R.reference(name))
    print(f"{name}: " + ", ".join(f"{k} {100 * v:.3f}%" for k, v in shares.items()))
    for k, v in shares.items():
        assert v <= R.AMBIGUITY_CAP, f"{k}: {100 * v:.2f}% of the results are ambiguous"


@pytest.mark.parametrize("name", R.CASES)
def test_anchor_oracle_equals_the_model_outside_the_band(name):
    ref = R.reference(name)
    unequal, errs = compare(oracle32(name), ref)
    print(f"{name}: err_oracle32 " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(v == 0 for v in unequal.values()), unequal
    # a few fp32 roundings, amplified by at most 1 / Z: 10 in reproject (Z >= 0.1), 100 in projmap (Z > 0.01)
    assert errs["reproject coords"] < 1e-4 and errs["projmap coords"] < 1e-3 and errs["iproj"] < 1e-5
    assert all(errs[f"frame_distance_{b}"] < 1e-5 for b in R.BETAS)


@pytest.mark.parametrize("name", R.CASES)
def test_inputs_contain_what_they_claim(name):
    c, ref = R.case(name), R.reference(name)
    z = ref["reproject"]["z"]
    below, valid = float((z < R.SUBST_Z).double().mean()), float(ref["reproject"]["valid"].double().mean())
    between = int(((z > R.SUBST_Z) & (z < R.PY_MIN_Z)).sum()), int(((z > R.PY_MIN_Z) & (z < R.KERNEL_MIN_Z)).sum())
    hist = torch.bincount(ref["depth_filter"]["count"].long().flatten(), minlength=7).tolist()
    print(f"{name}: reproject Z < 0.1 {100 * below:.1f}%, valid {100 * valid:.1f}%, in (0.1, 0.2) {between[0]}, in "
          f"(0.2, 0.25) {between[1]}; depth_filter counts 0..6 {hist}")
    assert 0.10 <= below <= 0.40 and 0.55 <= valid <= 0.90
    assert min(between) > 0
    pz = ref["projmap"]["z"]
    assert int(((pz > R.PY_MIN_Z) & (pz < R.KERNEL_MIN_Z)).sum()) > 0 and int((pz <= R.PROJMAP_EPS_Z).sum()) > 0
    assert len(hist) == 7 and min(hist) > 0, hist
    # zero disparities where they belong
    assert int((c["disps"] == 0).sum()) > 0 and int((c["df"]["disps"] == 0).sum()) > 0
    assert int((c["disps_nz"] == 0).sum()) == 0 and float(c["disps_nz"].min()) >= 0.05 and float(c["disps"].max()) <= 4.0
    # the poses: unit quaternions, the pi frame, the 2.5 rad frame, the negated one
    q = c["poses"][:, 3:].double()
    assert float((q.norm(dim=-1) - 1).abs().max()) < 1e-7
    assert abs(float(q[R.PI_FRAME, 3])) < 1e-7
    angle = 2 * torch.acos(q[:, 3].abs().clamp(max=1.0))
    assert abs(float(angle[R.BIG_FRAME]) - 2.5) < 0.2 and abs(float(angle[R.PI_FRAME]) - math.pi) < 1e-6
    rest = [k for k in range(R.NUM_FRAMES) if k not in (R.BIG_FRAME, R.PI_FRAME)]
    assert float(angle[rest].max()) < 0.3
    assert float(q[R.NEG_FRAME, 3]) < -0.9 and torch.equal(c["poses_plain"][R.NEG_FRAME, 3:], -c["poses"][R.NEG_FRAME, 3:])
    assert torch.equal(R.rotation(c["poses"][:, 3:]), R.rotation(c["poses_plain"][:, 3:]))
    # intrinsics: every frame its own row, every entry within +-20 % and at least 1 % from every other frame's
    K = c["intrinsics_frames"].double()
    assert float((K / c["intrinsics"].double() - 1).abs().max()) <= 0.2 + 1e-6
    gap = (K[:, None] / K[None] - 1).abs() + torch.eye(R.NUM_FRAMES)[..., None]
    assert float(gap.max(-1).values.min()) > 0.01
    # edges: all ordered pairs, then the stereo edges
    assert len(c["ii"]) == R.NUM_FRAMES * (R.NUM_FRAMES - 1) and int((c["ii_st"] == c["jj_st"]).sum()) == R.NUM_FRAMES
    # frame_distance takes both branches
    for beta in R.BETAS:
        far = ref[f"frame_distance_{beta}"]["far"]
        assert 10 <= int(far.sum()) <= len(far) - 10
    # depth_filter's buffer ends
    assert c["df"]["ix"].tolist() == [0, 1, 4, 8, 9] and c["df"]["disps"].shape[0] == 10


def test_frame_distance_known_answer_is_the_models():
    k = R.frame_distance_kat()
    m = R.frame_distance(k["poses"], k["disps"], k["intrinsics"], k["ii"], k["jj"], k["beta"])
    assert k["share"] == 0.75 and float(m["share"]) == 0.75 and not bool(m["far"]) and bool(m["amb"])
    assert abs(float(m["dist"]) - k["answer"]) < 1e-12 * k["answer"]
    k1 = R.frame_distance_kat(extra_far_pixels=1)
    m1 = R.frame_distance(k1["poses"], k1["disps"], k1["intrinsics"], k1["ii"], k1["jj"], k1["beta"])
    assert k1["share"] < 0.75 and bool(m1["far"]) and float(m1["dist"]) == R.FAR and not bool(m1["amb"])
    o1 = O.frame_distance(k1["poses"], k1["disps"], k1["intrinsics"], k1["ii"], k1["jj"], k1["beta"])
    assert float(o1) == R.FAR


def test_glue_references_are_the_update_steps_expressions():
    """The planted values do what they are planted for in the torch reference: clamped flows, +-inf to +-64, NaN kept."""
    g = R.glue_case()
    m = R.motion_features_reference(g["coords0"], g["coords1"], g["target"])
    E, ht, wd = R.GLUE_SHAPE
    assert m.shape == (E, 4, ht, wd) and m.dtype == torch.float16 and (E * ht * wd) % 256 != 0
    assert int(torch.isnan(m).sum()) >= 6 and int((m == 64).sum()) >= 4 and int((m == -64).sum()) >= 4
    assert not bool(torch.isinf(m).any())
    assert bool(torch.isnan(m[1, 0, 5, 5])) and bool(torch.isnan(m[1, 2, 5, 5])) and bool(torch.isnan(m[2, 2, 9, 9]))
    t, bt, bw = R.ba_inputs_reference(g["coords1"], g["delta"], g["weight"])
    assert bt.shape == (E, 2, ht, wd) and bool(torch.isnan(t).any()) and bool(torch.isinf(t).any())


# -------------------------------------------------------------------------------------------------- sensitivity ----
def _rewritten(fn, old, new, count=1):
    """`fn` recompiled in its own module's namespace with `old` replaced by `new` (exactly `count` times)."""
    src = textwrap.dedent(inspect.getsource(fn))
    assert src.count(old) == count, (fn.__name__, old, src.count(old))
    scope = {}
    exec(compile(src.replace(old, new), f"<{fn.__name__}: {old} -> {new}>", "exec"), fn.__globals__, scope)
    return scope[fn.__name__]


# name -> (attribute of geom_restatement, its wrong replacement, the operations to recompute)
def _mutations():
    fd = ("frame_distance",)
    return {
        "reproject: intrinsics of i and j swapped":
            ("reproject", _rewritten(R.reproject, "intrinsics[ii], intrinsics[jj]", "intrinsics[jj], intrinsics[ii]"),
             ("reproject",)),
        "relative pose M_i inv(M_j)":
            ("relative_poses", _rewritten(R.relative_poses, "M_j @ torch.linalg.inv(M_i)", "M_i @ torch.linalg.inv(M_j)"),
             ("reproject", "projmap", "frame_distance", "depth_filter")),
        "reproject valid at 0.25": ("PY_MIN_Z", 0.25, ("reproject",)),
        "projmap valid at 0.2": ("KERNEL_MIN_Z", 0.2, ("projmap",)),
        "reproject without the Z < 0.1 substitution":
            ("reproject", _rewritten(R.reproject, "torch.where(z < SUBST_Z, torch.ones_like(z), z)", "z"), ("reproject",)),
        "depth_filter: round for floor":
            ("depth_filter", _rewritten(R.depth_filter, "torch.floor(uj), torch.floor(vj)",
                                        "torch.round(uj), torch.round(vj)"), ("depth_filter",)),
        "depth_filter: u0 <= wd-1":
            ("depth_filter", _rewritten(R.depth_filter, "(u0 < wd - 1)", "(u0 <= wd - 1)"), ("depth_filter",)),
        "depth_filter: neighbours +-1, +-2, +-3": ("NEIGHBOURS", (-1, -2, -3, 1, 2, 3), ("depth_filter",)),
        "stereo baseline +0.1": ("STEREO_TX", -R.STEREO_TX, ("reproject",)),
        "frame_distance without the translation leg":
            ("frame_distance", _rewritten(R.frame_distance, "T[:, :3, :3] = torch.eye(3, dtype=F64)", "pass"), fd),
        "frame_distance: beta and 1 - beta swapped":
            ("frame_distance", _rewritten(R.frame_distance, "w_full, w_trans = beta, 1.0 - beta",
                                          "w_full, w_trans = 1.0 - beta, beta"), fd),
    }


def _model(name, ops):
    """The model of the listed operations on case `name`, computed afresh (under whatever patch is active)."""
    c = R.case(name)
    out = dict(R.reference(name))
    if "reproject" in ops:
        out["reproject"] = R.reproject(c["poses"], c["disps"], c["intrinsics_frames"], c["ii_st"], c["jj_st"])
    if "projmap" in ops:
        out["projmap"] = R.projmap(c["poses"], c["disps"], c["intrinsics"], c["ii"], c["jj"])
    if "frame_distance" in ops:
        for beta in R.BETAS:
            out[f"frame_distance_{beta}"] = R.frame_distance(c["poses"], c["disps"], c["intrinsics"], c["ii"], c["jj"], beta)
    if "depth_filter" in ops:
        out["depth_filter"] = R.depth_filter(**c["df"])
    return out


@pytest.mark.parametrize("name", R.CASES)
def test_checks_reject_subtly_wrong_models(name, monkeypatch):
    ref, got = R.reference(name), oracle32(name)
    unequal0, errs0 = compare(got, ref)
    assert all(v == 0 for v in unequal0.values())
    found = {}
    for label, (attr, wrong, ops) in _mutations().items():
        with monkeypatch.context() as mp:
            mp.setattr(R, attr, wrong)
            unequal, errs = compare(got, _model(name, ops), amb=ref)
        factor = max(errs[k] / R.bound(errs0[k]) for k in errs)
        found[label] = (sum(unequal.values()), factor)
    print(f"{name}: " + "; ".join(f"{k}: unequal {u}, err / bound {f:.3g}" for k, (u, f) in found.items()))
    unequal, errs = compare(got, _model(name, ("reproject", "projmap", "frame_distance", "depth_filter")))
    assert unequal == unequal0 and errs == errs0, "the patches are undone"
    for label, (u, f) in found.items():
        assert u > 0 or f >= 10.0, f"{label}: not caught (unequal {u}, err / bound {f:.3g})"


def test_known_answer_rejects_the_threshold_taken_inclusive(monkeypatch):
    k = R.frame_distance_kat()
    wrong = _rewritten(R.frame_distance, "far = share < FAR_SHARE", "far = share <= FAR_SHARE")
    m = wrong(k["poses"], k["disps"], k["intrinsics"], k["ii"], k["jj"], k["beta"])
    print(f"share {float(m['share'])}: `<=` gives {float(m['dist'])}, the known answer is {k['answer']:.6f}")
    assert bool(m["far"]) and float(m["dist"]) == R.FAR and math.isfinite(k["answer"]) and k["answer"] < 100
    # and it is this input alone that tells: on the seeded cases no share is within 1e-3 of 0.75
    for name in R.CASES:
        for beta in R.BETAS:
            assert float((R.reference(name)[f"frame_distance_{beta}"]["share"] - R.FAR_SHARE).abs().min()) > 1e-3
