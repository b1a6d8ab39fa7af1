"""Volume-to-volume registration and merge without a GPU: tests/tsdf_merge_restatement.py, which the MI355X tests hold
csrc/tsdf_merge.hip to bit for bit, is held here against independent definitions -- its Jacobian against central
differences of an fp64 residual, its sums against a plain fp64 J^T W J, its merge against the analytic room and against
the weighted mean in fp64 -- and against what it is for: from ten displaced starts it brings a second volume of a
three-plane room back onto the first.  Then the contract's skips, every host-side refusal of go_slam_amd/tsdf_merge.py,
the text round trip, the config key's refusal, and the two kernels' register, scratch and LDS budget (compile only)."""
import math
import os
import re
import shutil
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import tsdf_align_restatement as AR                            # noqa: E402
import tsdf_merge_restatement as MR                            # noqa: E402

CHUNK = 2048                     # the restatement takes it as an argument; any of the contract's sizes serves here
U32 = 2.0 ** -24
F = np.float32


def truth():
    """S-world to D-world: turned by 12 degrees about a generic axis and shifted by (0.3, -0.2, 0.1)."""
    axis = np.array([0.3, -0.5, 0.8])
    axis /= np.linalg.norm(axis)
    return np.concatenate([AR.rotation(axis * math.radians(12.0)), np.array([[0.3], [-0.2], [0.1]])], 1)


CENTRE = (0.55, 0.5, 1.5)                     # D-world: the corner region, every S lattice below lies inside D's box around it
S_COARSE = ((25, 23, 21), 0.05, 0.20)
S_FINE = ((31, 29, 27), 0.04, 0.16)
S_WIDE = ((41, 23, 21), 0.05, 0.20)           # 2 m along x: sticks out past D's far x face at 1.6 m


@pytest.fixture(scope="module")
def dest():
    tsdf, weight = AR.scene_volume(AR.PLANES_OFF)
    return MR.volume(tsdf, weight, AR.SCENE_LO, AR.SCENE_VOXEL, AR.SCENE_TRUNC)


def source(spec, centre=CENTRE, trunc=None):
    dims, voxel, tr = spec
    return MR.moved_room(dims, voxel, tr if trunc is None else trunc, truth(), AR.PLANES_OFF, centre)


# ---- the Jacobian ---------------------------------------------------------------------------------------------------
def residual64(D, S, pose, idx):
    """The residual of the contract in float64 at S's lattice points idx: trilinear tsdf_D at R p + o, minus tsdf_S times
    trunc_S / trunc_D."""
    p = np.asarray(S["lo"]) + idx * S["voxel"]
    g = (p @ pose[:, :3].T + pose[:, 3] - np.asarray(D["lo"])) / D["voxel"]
    a = np.floor(g).astype(np.int64)
    s = g - a
    t = D["tsdf"].astype(np.float64)
    out = np.zeros(len(idx))
    for i in (0, 1):
        for j in (0, 1):
            for k in (0, 1):
                wgt = (s[:, 0] if i else 1 - s[:, 0]) * (s[:, 1] if j else 1 - s[:, 1]) * (s[:, 2] if k else 1 - s[:, 2])
                out += wgt * t[a[:, 0] + i, a[:, 1] + j, a[:, 2] + k]
    fs = S["tsdf"][idx[:, 0], idx[:, 1], idx[:, 2]].astype(np.float64)
    return out - fs * (S["trunc"] / D["trunc"]), s


def test_jacobian_equals_central_differences_of_the_fp64_residual(dest):
    """Perturbation as the step applies it: o + v, exp(omega) R.  The transform is 5 cm / 3 degrees off the truth so that
    residuals and gradients are generic; S has another voxel and truncation than D (ratio 0.8)."""
    S, _, _ = source(S_FINE)
    pose = MR.displaced_transform(truth(), 0.05, 3.0, np.random.default_rng(2))
    t = MR.sample_terms(dest, S, pose, 1)
    idx = t["idx"]
    r0, frac = residual64(dest, S, pose, idx)
    h = 1e-6                                      # metres and radians: a point moves by at most 3 h = 6e-5 cells
    inner = ((frac > 1e-3) & (frac < 1 - 1e-3)).all(1) & t["valid"]          # the differences must stay inside one cell
    assert inner.sum() > 2500
    fd = np.zeros((len(idx), 6))
    for i in range(6):
        e = np.zeros(6)
        e[i] = h
        plus = np.concatenate([AR.rotation(e[3:]) @ pose[:, :3], (pose[:, 3] + e[:3])[:, None]], 1)
        minus = np.concatenate([AR.rotation(-e[3:]) @ pose[:, :3], (pose[:, 3] - e[:3])[:, None]], 1)
        fd[:, i] = (residual64(dest, S, plus, idx)[0] - residual64(dest, S, minus, idx)[0]) / (2 * h)
    # Tolerance, DESIGN section 28's derivation with lattice points in the place of pixels.  The restated gradient n is
    # a difference of two doubly lerped corner values, all |.| <= 1: each of its ~8 operations rounds by at most 2^-24,
    # e_n = 8 * 2^-24.  Its sample point is computed in fp32 too: p = lo_S + idx * voxel_S, q = R p, pw = q + o and g =
    # (pw - lo_D) / voxel_D are ~8 roundings of relative size 2^-24 at |g| <= 45 cells (D's longest axis), dg = 8 * 2^-24
    # * 45 cells per axis, and the trilinear gradient changes by at most the largest mixed second difference of a cell's
    # corners per cell moved; corner values of this room differ by at most voxel_D / trunc_D = 0.25 per step, which
    # bounds that second difference.  So |n - n_exact| <= e_n + 3 * dg * 0.25, gw = n / voxel_D, and the rotation entries
    # q x gw carry |q| <= 3 m on each of two products plus the fp32 rounding of q itself against |gw| <= 5 sqrt(3).
    # The central difference adds its own fp64 rounding 2^-53 * |r| / h <= 2.4e-10 and no truncation error to speak of.
    # The residual itself must agree to the lerp roundings, the slope times dg, and the rounding of fs * ratio.
    e_n = 8 * U32 + 3 * (8 * U32 * 45) * 0.25
    tol_t = e_n / dest["voxel"] + 4e-10
    qmax = float(np.abs(t["q"][inner]).max())
    assert qmax <= 3.0
    tol_r = 2 * qmax * tol_t + 2 * (4 * U32 * qmax) * 5 * math.sqrt(3) + 4e-10
    J = t["J"].astype(np.float64)
    err_t = np.abs(J[inner, :3] - fd[inner, :3]).max()
    err_r = np.abs(J[inner, 3:] - fd[inner, 3:]).max()
    err_f = np.abs(t["f"][inner].astype(np.float64) - r0[inner]).max()
    print(f"{inner.sum()} samples: |J - fd| translation {err_t:.3e} (tol {tol_t:.3e}), rotation {err_r:.3e} (tol {tol_r:.3e}), "
          f"|r - r64| {err_f:.3e}; largest |J| {np.abs(J[inner]).max():.3f}")
    assert np.abs(fd[inner]).max() > 1.0                        # the comparison is not between zeros
    assert err_t <= tol_t and err_r <= tol_r
    assert err_f <= e_n + 3 * U32                               # + fl(trunc_S / trunc_D), fl(fs * ratio), fl(f - fr)


def test_sums_equal_a_plain_fp64_normal_system(dest):
    """H, b, cost and sq against np.einsum over the same fp32 J, wt and r, within n * 2^-52 relative per entry (of the
    entry itself, and of the sum of the terms' magnitudes)."""
    S, _, _ = source(S_FINE)
    pose = MR.displaced_transform(truth(), 0.08, 4.0, np.random.default_rng(4))
    for stride, huber in ((1, 0.5), (2, 0.05), (3, 0.5)):
        t = MR.sample_terms(dest, S, pose, stride, huber=huber)
        row = MR.system(dest, S, pose[None], stride, CHUNK, huber=huber)[0]
        v = t["valid"]
        J, f, w = t["J"][v].astype(np.float64), t["f"][v].astype(np.float64), t["wt"][v].astype(np.float64)
        n = int(v.sum())
        assert row[28] == n and row[30] == t["considered"].sum() and n > 300 and row[31] == 0
        assert huber == 0.5 or (w < 1).any()
        H = np.einsum("s,si,sj->ij", w, J, J)
        Habs = np.einsum("s,si,sj->ij", w, np.abs(J), np.abs(J))
        at, worst = 0, 0.0
        for i in range(6):
            for j in range(i, 6):
                assert abs(row[at] - H[i, j]) <= n * 2.0 ** -52 * abs(H[i, j]), (i, j)
                assert abs(row[at] - H[i, j]) <= n * 2.0 ** -52 * Habs[i, j], (i, j)
                worst = max(worst, abs(row[at] - H[i, j]) / (n * 2.0 ** -52 * abs(H[i, j])))
                at += 1
            bi = (w * J[:, i] * f).sum()
            assert abs(row[21 + i] - bi) <= n * 2.0 ** -52 * abs(bi), i
            worst = max(worst, abs(row[21 + i] - bi) / (n * 2.0 ** -52 * abs(bi)))
        print(f"stride {stride}, huber {huber}: n = {n}, largest error {worst:.4f} of n 2^-52 |entry|")
        assert abs(row[27] - (w * f * f).sum()) <= n * 2.0 ** -52 * row[27]
        assert abs(row[29] - (f * f).sum()) <= n * 2.0 ** -52 * row[29]


# ---- convergence ----------------------------------------------------------------------------------------------------
def run_starts(D, S, seed):
    rng = np.random.default_rng(seed)
    starts = np.stack([MR.displaced_transform(truth(), 0.05, 3.0, rng) for _ in range(6)] +
                      [MR.displaced_transform(truth(), 0.10, 5.0, rng) for _ in range(4)])
    pose, rows, trace = MR.register(D, S, starts, CHUNK, levels=((2, 10), (1, 10)))
    errs = np.array([AR.pose_error(p, truth()) for p in pose])
    pairs = np.array([AR.pose_error(p, q) for i, p in enumerate(pose) for q in pose[i + 1:]])
    return pose, rows, trace, errs, pairs


def assert_converged(S, rows, trace, errs, pairs, D):
    """Section 28's bounds: every pair of ends within 1e-5 m, every end within a tenth of the finer voxel and 0.1 degrees
    of the truth (the offset is the bias of the cells that straddle a crease)."""
    assert (trace[:, :, 3] == 1).all()
    assert pairs[:, 0].max() <= 1e-5
    assert errs[:, 0].max() <= min(S["voxel"], D["voxel"]) / 10 and errs[:, 1].max() <= 0.1


@pytest.mark.parametrize("spec", [S_COARSE, S_FINE])
def test_every_start_ends_at_one_point_near_the_truth(dest, spec):
    """Six starts at 5 cm / 3 degrees and four at 10 cm / 5 degrees, levels ((2, 10), (1, 10)).  Measured with this
    restatement: 25 x 23 x 21 at 5 cm ends 1.05 mm / 0.029 degrees from the truth, 31 x 29 x 27 at 4 cm (truncation 0.16 m:
    ratio 0.8) 0.67 mm / 0.015 degrees, every start within 1e-7 m of every other.  S lies inside D's box and its band
    inside D's band, so every considered sample is used."""
    S, _, _ = source(spec)
    pose, rows, trace, errs, pairs = run_starts(dest, S, 31)
    print(spec, "error:", errs[:, 0].max(), "m,", errs[:, 1].max(), "deg; largest distance between two ends", pairs[:, 0].max(),
          "m,", pairs[:, 1].max(), "deg; count", rows[0, 28], "of", rows[0, 30])
    assert_converged(S, rows, trace, errs, pairs, dest)
    assert (rows[:, 28] == rows[:, 30]).all() and (rows[:, 28] > 5000).all()


def test_a_source_that_sticks_out_of_the_destination_still_converges(dest):
    """41 points along x reach past D's far x face: the floor's and the wall's band go on there, so those samples are
    considered and find no cell."""
    S, _, _ = source(S_WIDE, centre=(0.95, 0.5, 1.5))
    pose, rows, trace, errs, pairs = run_starts(dest, S, 32)
    print("error:", errs[:, 0].max(), "m,", errs[:, 1].max(), "deg; spread", pairs[:, 0].max(), "count", rows[0, 28], "of",
          rows[0, 30])
    assert (0 < rows[:, 28]).all() and (rows[:, 28] < rows[:, 30]).all()
    assert_converged(S, rows, trace, errs, pairs, dest)


# ---- the merge against the analytic room ----------------------------------------------------------------------------
def test_merge_into_an_empty_volume_reproduces_the_analytic_room(dest):
    """S at 4 cm with the truncation the contract demands (0.2 m >= D's) merged into an empty D at the true transform.  A
    cell of S is clean when its eight corners are unsaturated and nearest to the same plane: the room's distance is then
    linear over the cell and the trilinear value exact, so the merged tsdf at a point of D in such a cell is
    clip(sdf / trunc_D) up to rounding."""
    S, plane, sdf_s = source(S_FINE, trunc=0.2)
    with pytest.raises(ValueError):
        MR.merge(MR.empty_volume(dest["tsdf"].shape, dest["lo"], dest["voxel"], dest["trunc"]), source(S_FINE)[0],
                 MR.inverse(truth()))                                               # 0.16 into 0.2
    D0 = MR.empty_volume(dest["tsdf"].shape, dest["lo"], dest["voxel"], dest["trunc"], colors=False)
    d2s = MR.inverse(truth())
    out = MR.merge(D0, S, d2s)
    dims = D0["tsdf"].shape
    idx = MR.strided_samples(dims, 1)
    p = np.asarray(D0["lo"]) + idx * D0["voxel"]                                     # fp64
    g = ((p @ d2s[:, :3].T + d2s[:, 3]) - np.asarray(S["lo"])) / S["voxel"]
    a = np.floor(g).astype(np.int64)
    inside = ((a >= 0) & (a < np.asarray(S["tsdf"].shape) - 1)).all(1)
    a = np.where(inside[:, None], a, 0)
    clean = inside.copy()
    first = plane[a[:, 0], a[:, 1], a[:, 2]]
    for i in (0, 1):
        for j in (0, 1):
            for k in (0, 1):
                clean &= np.abs(sdf_s[a[:, 0] + i, a[:, 1] + j, a[:, 2] + k]) < S["trunc"]
                clean &= plane[a[:, 0] + i, a[:, 1] + j, a[:, 2] + k] == first
    frac = g - np.floor(g)
    clean &= ((frac > 1e-3) & (frac < 1 - 1e-3)).all(1)           # the fp32 point falls into the same cell as the fp64 one
    want = np.clip(MR.room_sdf(p, AR.PLANES_OFF) / D0["trunc"], -1.0, 1.0)
    got = out["tsdf"].reshape(-1).astype(np.float64)
    # Bound.  g is reached through p = lo_D + idx * voxel_D (2 roundings), the transform's entries rounded to fp32 (4 per
    # row), three products and three sums per row (6), lo_S rounded to fp32 (1), the difference and the quotient (2): 15,
    # say 16, roundings of relative size 2^-24 on magnitudes of at most M metres, the largest coordinate in either
    # frame.  The three axes' errors meet the plane's unit normal: a factor sqrt(3).  A metre is 1 / trunc_D of the
    # tsdf.  Then the values: S's stored corner (1), seven lerps of three roundings each on |.| <= 2, ratio, product,
    # and (s * ws) / ws (2): 32 roundings of 2^-24 at most.  In cells: 2^-24 times a lattice coordinate of about 60
    # (M / voxel_S) times voxel_S / trunc_D = 0.2, times 16 sqrt(3).
    M = max(np.abs(p).max(), np.abs(p @ d2s[:, :3].T + d2s[:, 3]).max(), np.abs(S["lo"]).max(), np.abs(d2s[:, 3]).max())
    assert M <= 2.6
    bound = (math.sqrt(3) * 16 * M / D0["trunc"] + 32) * U32
    err = np.abs(got - want)[clean]
    print(f"{clean.sum()} clean points, largest error {err.max():.3e} (bound {bound:.3e}); touched {out['touched'].sum()}")
    assert clean.sum() > 4000
    assert out["touched"].reshape(-1)[clean].all()
    assert err.max() <= bound
    assert np.array_equal(out["weight"].reshape(-1)[clean], np.ones(clean.sum(), F))     # the trilinear weight of ones
    untouched = ~out["touched"]
    assert np.array_equal(out["tsdf"][untouched], D0["tsdf"][untouched]) and not out["weight"][untouched].any()


# ---- the weighted mean, the order, the skips --------------------------------------------------------------------------
EXACT_DIMS, EXACT_LO, EXACT_VOXEL = (9, 7, 11), (-0.5, 0.25, -1.0), 0.125      # exact in binary: g = idx, fractions 0


def random_volume(seed, trunc=0.5, whole=True):
    """Weights 1 .. 5: whole numbers (sums of them are exact) or not."""
    rng = np.random.default_rng(seed)
    weight = rng.integers(1, 6, EXACT_DIMS) if whole else rng.uniform(1.0, 5.0, EXACT_DIMS)
    return MR.volume(rng.uniform(-0.9, 0.9, EXACT_DIMS), weight, EXACT_LO, EXACT_VOXEL, trunc,
                     rng.uniform(0, 1, (3,) + EXACT_DIMS))


def interior():
    m = np.zeros(EXACT_DIMS, bool)
    m[:-1, :-1, :-1] = True
    return m


def test_identity_merge_on_one_lattice_is_the_weighted_mean():
    """On a lattice whose coordinates are exact in binary every point of D is a corner of S with fractions 0, and the
    trilinear value is the corner's bits.  The merged value is (t_D w_D + t_S w_S) / (w_D + w_S) with five fp32 roundings
    (two products, their sum, w_D + w_S -- exact here, small integers -- and the quotient): within 5 * 2^-24 of the fp64
    mean, as |t| <= 1.  It is not bit-equal to it; even into an empty volume (s * w) / w rounds twice.  The far faces
    stay as they were: their points are corners of no cell."""
    D, S = random_volume(1), random_volume(2)
    out = MR.merge(D, S)
    m = interior()
    assert np.array_equal(out["touched"], m)
    d, s = {k: D[k].astype(np.float64) for k in ("tsdf", "weight", "colors")}, {k: S[k].astype(np.float64) for k in
                                                                                 ("tsdf", "weight", "colors")}
    mean = (d["tsdf"] * d["weight"] + s["tsdf"] * s["weight"]) / (d["weight"] + s["weight"])
    cmean = (d["colors"] * d["weight"] + s["colors"] * s["weight"]) / (d["weight"] + s["weight"])
    err = np.abs(out["tsdf"].astype(np.float64) - mean)[m].max()
    cerr = np.abs(out["colors"].astype(np.float64) - cmean)[:, m].max()
    print("largest error against the fp64 mean:", err, "colours", cerr, "; bit-equal to its fp32 rounding:",
          (out["tsdf"][m] == mean[m].astype(F)).mean())
    assert err <= 5 * U32 and cerr <= 5 * U32
    assert np.array_equal(out["weight"][m], (D["weight"] + S["weight"])[m])
    for name in ("tsdf", "weight"):
        assert np.array_equal(out[name][~m].view(np.int32), D[name][~m].view(np.int32))
    assert np.array_equal(out["colors"][:, ~m].view(np.int32), D["colors"][:, ~m].view(np.int32))
    empty = MR.empty_volume(EXACT_DIMS, EXACT_LO, EXACT_VOXEL, 0.5)
    first = MR.merge(empty, S)
    assert np.abs(first["tsdf"].astype(np.float64) - s["tsdf"])[m].max() <= 2 * U32
    assert np.array_equal(first["weight"][m], S["weight"][m])


def test_the_order_of_two_merges_matters_to_rounding_only():
    """Each merge is within 5 * 2^-24 of the exact weighted mean of what it was given (the weights are no whole numbers
    here, so w_D + w_S rounds as well: it is one of the five), and passes an error in D's value on with a factor w_D /
    (w_D + w_S) <= 1 and a relative error of D's weight with a factor <= 1 too: after two merges either order is within
    10 * 2^-24 of the exact mean of the three, the two orders within 20 * 2^-24 of each other.  Below the weight cap."""
    A, B = random_volume(3, whole=False), random_volume(4, whole=False)
    base = random_volume(7, whole=False)                        # into an empty volume the first merge is (s * w) / w: no test
    empty = MR.empty_volume(EXACT_DIMS, EXACT_LO, EXACT_VOXEL, 0.5)
    ab, ba = MR.merge(MR.merge(base, A), B), MR.merge(MR.merge(base, B), A)
    m = interior()
    assert np.abs(ab["weight"] - ba["weight"]).max() <= 2 * U32 * 15 and ab["weight"].max() <= 15 < 64
    diff = np.abs(ab["tsdf"].astype(np.float64) - ba["tsdf"])[m].max()
    cdiff = np.abs(ab["colors"].astype(np.float64) - ba["colors"])[:, m].max()
    print("largest difference between the two orders:", diff, "colours", cdiff)
    assert diff <= 20 * U32 and cdiff <= 20 * U32
    assert diff > 0                                             # and it does matter to rounding
    C = random_volume(3)
    capped = MR.merge(MR.merge(empty, C, max_weight=4.0), C, max_weight=4.0)
    assert capped["weight"][m].max() == 4.0 and (capped["weight"][m] == np.minimum(2 * C["weight"], 4)[m]).all()


def test_skipped_points_keep_their_bits():
    D, S = random_volume(5), random_volume(6)
    S["weight"][4, 3, 5] = 0.5                                   # one corner below min_weight: its eight cells are skipped
    S["tsdf"][1, 1, 1] = -0.95                                   # with ratio 1.1: s = -1.045 < -1 (every other |s| <= 0.99)
    S["tsdf"][2, 2, 2] = 0.95                                    # s = 1.045: held at 1
    S["trunc"] = 0.55
    out = MR.merge(D, S)
    m = interior()
    expect = m.copy()
    expect[3:5, 2:4, 4:6] = False
    expect[1, 1, 1] = False
    assert np.array_equal(out["touched"], expect)
    for name in ("tsdf", "weight"):
        assert np.array_equal(out[name][~expect].view(np.int32), D[name][~expect].view(np.int32))
    assert np.array_equal(out["colors"][:, ~expect].view(np.int32), D["colors"][:, ~expect].view(np.int32))
    assert (out["tsdf"][expect] != D["tsdf"][expect]).mean() > 0.99
    fresh = MR.merge(MR.empty_volume(EXACT_DIMS, EXACT_LO, EXACT_VOXEL, 0.5), S)
    assert fresh["tsdf"][2, 2, 2] == 1.0 and fresh["touched"][2, 2, 2]          # fminf(1, s), then (1 * w) / w
    assert np.array_equal(MR.merge(D, S, min_weight=0.5)["touched"][3:5, 2:4, 4:6], np.ones((2, 2, 2), bool))
    with pytest.raises(ValueError):
        MR.merge(S, D)                                           # 0.5 into 0.55
    nocol = {k: v for k, v in D.items() if k != "colors"}
    plain = MR.merge(nocol, S)
    assert "colors" not in plain and np.array_equal(plain["tsdf"], out["tsdf"])


def test_considered_needs_both_truncations_and_the_weight():
    """A sample counts with weight_S >= min_weight, |f_S| < 1 and |f_S * ratio| < 1; only then can it be used."""
    D = MR.volume(np.full((5, 5, 5), 0.25), np.ones((5, 5, 5)), (0, 0, 0), 0.125, 0.4)
    S = MR.volume(np.full((3, 3, 3), 0.5), np.ones((3, 3, 3)), (0.0625, 0.0625, 0.0625), 0.125, 0.4)
    eye = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)
    assert MR.system(D, S, eye[None], 1, CHUNK)[0, [28, 30]].tolist() == [27, 27]
    assert MR.system(D, S, eye[None], 2, CHUNK)[0, [28, 30]].tolist() == [8, 8]
    S["weight"][0, 0, 0] = 0.5
    S["tsdf"][1, 1, 1] = 1.0
    S["tsdf"][2, 2, 2] = -1.0
    assert MR.system(D, S, eye[None], 1, CHUNK)[0, [28, 30]].tolist() == [24, 24]
    S["trunc"] = 0.9                                             # ratio 2.25: 0.5 * 2.25 >= 1 everywhere
    assert MR.system(D, S, eye[None], 1, CHUNK)[0, [28, 30]].tolist() == [0, 0]
    S["trunc"], D["tsdf"][:] = 0.4, 1.0                          # D saturated: considered, not used
    assert MR.system(D, S, eye[None], 1, CHUNK)[0, [28, 30]].tolist() == [0, 24]
    D["tsdf"][:] = 0.25
    row = MR.system(D, S, eye[None], 1, CHUNK, huber=0.125)[0]   # r = 0.25 - 0.5: weight huber / |r| = 0.5
    assert row[27] == 24 * 0.5 * 0.0625 and row[29] == 24 * 0.0625


# ---- go_slam_amd/tsdf_merge.py on the host ----------------------------------------------------------------------------
@pytest.fixture()
def no_library(monkeypatch):
    from go_slam_amd import _lib

    def refuse():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "lib", refuse)


def host_volume(dims=(5, 4, 6), lo=(0.0, 0.0, 0.0), voxel=0.1, trunc=0.4, max_weight=64.0):
    from go_slam_amd.tsdf import TSDFVolume
    vol = TSDFVolume.__new__(TSDFVolume)
    vol.voxel, vol.lo, vol.dims, vol.trunc, vol.max_weight = voxel, np.array(lo, np.float64), dims, trunc, max_weight
    vol.device = torch.device("cpu")
    vol.tsdf, vol.weight, vol.colors = torch.ones(dims), torch.zeros(dims), torch.zeros((3,) + dims)
    vol._flags = "kept"
    return vol


def test_every_host_side_refusal(no_library):
    from go_slam_amd import tsdf_merge as TM
    a, b = host_volume(), host_volume(trunc=0.5)
    eye = np.eye(4)
    shear = np.eye(4)
    shear[0, 1] = 0.1
    mirror = np.diag([1.0, 1.0, -1.0, 1.0])
    bad_register = [dict(src=a), dict(src=types.SimpleNamespace()), dict(T_init=np.zeros((2, 2))), dict(T_init=eye * math.nan),
                    dict(T_init=shear), dict(T_init=mirror), dict(T_init=np.zeros((1, 4, 3))),
                    dict(levels=()), dict(levels=((0, 5),)), dict(levels=((2, -1),)), dict(levels=((1.5, 2),)),
                    dict(levels=(4, 10)), dict(huber=0.0), dict(huber=-0.5), dict(huber=math.nan), dict(min_weight=math.nan),
                    dict(lam_rel=-1e-6), dict(lam_rel=math.inf), dict(lam_abs=math.nan), dict(lam_abs=-1.0),
                    dict(min_count=0), dict(min_count=2.5), dict(min_count=True)]
    for bad in bad_register:
        args = dict(dict(src=b, T_init=eye), **bad)
        with pytest.raises(ValueError, match="register_volumes"):
            TM.register_volumes(a, **args)
        with pytest.raises(ValueError, match="register_volumes"):
            a.register(args["src"], **{k: v for k, v in args.items() if k != "src"})
    other_device = host_volume()
    other_device.device = torch.device("meta")
    with pytest.raises(ValueError, match="register_volumes"):
        TM.register_volumes(a, other_device, eye)
    bad_merge = [dict(other=a), dict(other=types.SimpleNamespace()), dict(other=host_volume(trunc=0.39)), dict(T=shear),
                 dict(T=np.zeros((3, 3))), dict(T=np.stack([eye, eye])), dict(T=np.full((4, 4), math.inf)), dict(min_weight=0.0),
                 dict(min_weight=-1.0), dict(min_weight=math.nan), dict(other=other_device)]
    for bad in bad_merge:
        args = dict(dict(other=b), **bad)
        with pytest.raises(ValueError, match="TSDFVolume.merge"):
            a.merge(**args)
    assert a._flags == "kept"                                   # a refused merge has not touched the volume
    with pytest.raises(ValueError, match="smaller than this one's"):
        host_volume(trunc=0.2).merge(host_volume(trunc=0.16))    # 0.16 into 0.2
    for bad in (dict(volumes=[]), dict(transforms=[eye]), dict(transforms=[eye, shear]), dict(volumes=[a, object()])):
        args = dict(dict(volumes=[a, b], transforms=[eye, eye]), **bad)
        with pytest.raises(ValueError, match="union_volume"):
            TM.union_volume(**args)
    for bad in (dict(volumes=[]), dict(T_inits=[eye]), dict(T_inits=[None, np.stack([eye, eye])]), dict(T_inits=[None, shear])):
        args = dict(dict(volumes=[a, b], T_inits=None), **bad)
        with pytest.raises(ValueError, match="join_volumes"):
            TM.join_volumes(**args)


def test_union_volume_encloses_every_moved_box():
    from go_slam_amd import tsdf_merge as TM
    a = host_volume(dims=(11, 9, 13), lo=(-0.3, 0.2, 1.0), voxel=0.1, trunc=0.4, max_weight=32.0)
    b = host_volume(dims=(21, 17, 9), lo=(0.5, -1.0, 0.0), voxel=0.05, trunc=0.3, max_weight=64.0)
    T = np.eye(4)
    T[:3, :] = truth()
    u = TM.union_volume([a, b], [None, T], device="cpu")
    assert u.voxel == 0.05 and u.trunc == 0.3 and u.max_weight == 64.0 and u.device == torch.device("cpu")
    assert float(u.weight.max()) == 0 and float(u.tsdf.min()) == 1
    hi = u.lo + (np.asarray(u.dims) - 1) * u.voxel
    for vol, m in ((a, np.eye(4)[:3]), (b, T[:3])):
        box = TM.moved_box(vol, m)
        assert box.shape == (8, 3) and (box >= u.lo - 1e-12).all() and (box <= hi + 1e-12).all()
    lo_b = np.asarray(b.lo)
    far = lo_b + (np.asarray(b.dims) - 1) * b.voxel
    assert np.abs(TM.moved_box(b, T[:3])[7] - (T[:3, :3] @ far + T[:3, 3])).max() <= 1e-15
    tight = np.concatenate([TM.moved_box(a, np.eye(4)[:3]), TM.moved_box(b, T[:3])])
    assert np.abs(u.lo - tight.min(0)).max() <= 1e-12 and (hi - tight.max(0) < u.voxel + 1e-12).all()
    chosen = TM.union_volume([a, b], [None, T], voxel_size=0.2, trunc=0.25, max_weight=8.0, device="cpu")
    assert chosen.voxel == 0.2 and chosen.trunc == 0.25 and chosen.max_weight == 8.0
    shift = np.eye(4)
    shift[0, 3] = 60.0                                          # 60 m at 5 cm: 1200 points
    with pytest.raises(ValueError, match="at most 1024"):
        TM.union_volume([a, b], [None, shift], device="cpu")
    assert TM.union_volume([a, b], [None, shift], voxel_size=0.1, device="cpu").dims[0] <= 1024


def test_merge_text_round_trip_bit_for_bit():
    from go_slam_amd import tsdf_merge as TM
    rep = {"T": np.eye(4), "ok": True, "registered": True, "overlap": 1 / 3, "rmse_m": 2.0 ** -40, "moved_m": 0.30000000000000004,
           "moved_deg": 179.99999999999997, "moved_constrained_m": 5e-324, "n_constrained": 3, "count": 123456}
    result = TM.merge_report(rep)
    assert list(result) == list(TM.MERGE_REPORT_ORDER) and result["ok"] == 1 and result["count"] == 123456
    T = np.concatenate([AR.rotation([0.1, -0.2, 0.3]), np.array([[1e-300], [-1 / 3], [12345.678]])], 1)
    text = TM.merge_text(result, T)
    back, Tb = TM.parse_merge(text)
    assert list(back) == list(TM.MERGE_REPORT_ORDER)
    assert all(np.float64(back[k]).view(np.int64) == np.float64(result[k]).view(np.int64) for k in back)
    assert all(isinstance(back[k], int) for k in ("ok", "registered", "n_constrained", "count"))
    assert np.array_equal(Tb.view(np.int64), T.view(np.int64))
    assert TM.merge_text(back, Tb) == text
    given = TM.merge_report({"registered": False, "ok": True})
    assert given["ok"] == 1 and given["registered"] == 0 and math.isnan(given["overlap"]) and given["count"] == 0
    back, _ = TM.parse_merge(TM.merge_text(given, np.eye(4)))
    assert math.isnan(back["rmse_m"]) and back["registered"] == 0
    with pytest.raises(ValueError):
        TM.parse_merge("something else\n")


def test_merge_key_is_refused_before_anything_is_fused_or_written(tmp_path):
    """tsdf.merge with a missing or unreadable volume, or a bad init, raises before the video is touched: the namespace has
    no video, no output directory is written."""
    from go_slam_amd.tsdf import fuse_from_config
    cfg = {"mode": "rgbd", "mapping": {"bound": [[0, 1], [0, 1], [0, 1]]},
           "tsdf": {"enable": True, "merge": {"enable": True, "volume": str(tmp_path / "nothing.npz")}}}
    slam = types.SimpleNamespace(cfg=cfg, output=str(tmp_path / "out"), mode="rgbd")
    with pytest.raises(ValueError, match="tsdf.merge.volume .* is no file"):
        fuse_from_config(slam)
    cfg["tsdf"]["merge"]["volume"] = None
    with pytest.raises(ValueError, match="is no file"):
        fuse_from_config(slam)
    junk = tmp_path / "junk.npz"
    junk.write_bytes(b"not an archive")
    cfg["tsdf"]["merge"]["volume"] = str(junk)
    with pytest.raises(ValueError, match="cannot be read as a saved volume"):
        fuse_from_config(slam)
    short = tmp_path / "short.npz"
    np.savez(str(short), tsdf=np.ones((2, 2, 2), np.float32))
    cfg["tsdf"]["merge"]["volume"] = str(short)
    with pytest.raises(ValueError, match="cannot be read as a saved volume"):
        fuse_from_config(slam)
    good = tmp_path / "good.npz"
    host_volume().save(str(good))
    cfg["tsdf"]["merge"].update(volume=str(good), init=[[1, 0, 0], [0, 1, 0]])
    with pytest.raises(ValueError, match="tsdf.merge.init"):
        fuse_from_config(slam)
    assert not os.path.exists(slam.output)
    cfg["tsdf"]["merge"].update(init=np.eye(4).tolist())
    with pytest.raises(AttributeError):                         # a readable volume: it goes on to the video
        fuse_from_config(slam)
    cfg["tsdf"]["merge"]["enable"] = False
    cfg["tsdf"]["merge"]["volume"] = str(tmp_path / "nothing.npz")
    with pytest.raises(AttributeError):                         # without the key the file is not looked at, as before
        fuse_from_config(slam)
    assert not os.path.exists(slam.output)


def test_workspace_size_needs_no_gpu(built_lib):
    from go_slam_amd import _lib
    L = _lib.lib()
    C = L.gs_tsdf_align_chunk()
    assert L.gs_tsdf_register_workspace_bytes(1, 2, 2, 2, 1) == 256
    assert L.gs_tsdf_register_workspace_bytes(3, 64, 64, 64, 1) == 3 * (64 ** 3 // C) * 256
    assert L.gs_tsdf_register_workspace_bytes(3, 64, 64, 64, 4) == 3 * -(-(16 ** 3) // C) * 256
    assert L.gs_tsdf_register_workspace_bytes(2, 7, 9, 11, 5) == 2 * 256                     # 2 * 2 * 3 = 12 samples
    assert L.gs_tsdf_register_workspace_bytes(0, 7, 9, 11, 5) == 0
    for bad in ((-1, 4, 4, 4, 1), (1, 1, 4, 4, 1), (1, 4, 1025, 4, 1), (1, 4, 4, 0, 1), (1, 4, 4, 4, 0), (1, 4, 4, 4, -1),
                (1 << 13, 1024, 1024, 1024, 1)):
        assert L.gs_tsdf_register_workspace_bytes(*bad) == 0, bad


# ---- the kernels' budget (compile only) -------------------------------------------------------------------------------
def test_merge_kernels_fit_their_budget(tmp_path):
    """tsdf_register_system_kernel is tsdf_align_system_kernel's shape: a gather with 29 fp64 accumulators, four waves per
    SIMD, at most 128 VGPRs, no spilled accumulator, 4 x 32 doubles of LDS.  tsdf_merge_kernel is a streaming pass over D
    with up to 40 gathers of S in flight: eight waves per SIMD need at most 64 VGPRs; no LDS, no scratch."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "go_slam_amd", "csrc")
    out = tmp_path / "k.s"
    res = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-gpu-rdc",
                          "-munsafe-fp-atomics", "-I", csrc, "-I", os.path.join(ROOT, "include"), "--cuda-device-only", "-S",
                          os.path.join(csrc, "tsdf_merge.hip"), "-o", str(out)],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-2000:]
    assert "failed to meet occupancy target" not in res.stdout, res.stdout[-2000:]
    pat = re.compile(r"\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.name:\s+(\S+)\n(?:.*\n)*?"
                     r"\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)")
    budgets = {"tsdf_register_system_kernel": (128, 4 * 32 * 8), "tsdf_register_sum_kernel": (128, 0),
               "tsdf_merge_kernelILb1": (64, 0), "tsdf_merge_kernelILb0": (64, 0)}
    seen = set()
    for m in pat.finditer(open(out).read()):
        lds, name, scratch, vgpr = int(m.group(1)), m.group(2), int(m.group(3)), int(m.group(4))
        for key, (max_vgpr, max_lds) in budgets.items():
            if key in name:
                seen.add(key)
                print(name, "VGPRs", vgpr, "LDS", lds, "scratch", scratch)
                assert scratch == 0 and vgpr <= max_vgpr and lds <= max_lds, (name, scratch, vgpr, lds)
    assert seen == set(budgets)
