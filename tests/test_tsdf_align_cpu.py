"""SDF pose alignment without a GPU: tests/tsdf_align_restatement.py, which the MI355X tests hold csrc/tsdf_align.hip to
bit for bit, is held here against independent definitions -- its Jacobian against central differences of an fp64
residual, its chunked sums against a plain fp64 J^T W J, its retraction against orthogonality and the exponential -- and
against what it is for: from 30 displaced starts it returns to the true pose of a three-plane room.  Then the contract's
corner cases, every host-side refusal of go_slam_amd/localize.py, the file and text round trips, and the kernel's
register, scratch and LDS budget (compile only)."""
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

CHUNK = 2048                     # the restatement takes it as an argument; any of the contract's sizes serves here
U32, U64 = 2.0 ** -24, 2.0 ** -53


def room(planes):
    tsdf, weight = AR.scene_volume(planes)
    truth = AR.scene_pose()
    return tsdf, weight, truth, AR.scene_depth(truth, planes)


# ---- the Jacobian ---------------------------------------------------------------------------------------------------
def residual64(tsdf, depth_map, pose, iu, iv):
    """The residual of the contract in float64 on the same lattice, at given pixels: trilinear tsdf at R pc + o."""
    fx, fy, cx, cy = AR.SCENE_INTR
    d = depth_map[iv, iu].astype(np.float64)
    pc = np.stack([(iu - cx) / fx * d, (iv - cy) / fy * d, d], 1)
    g = (pc @ pose[:, :3].T + pose[:, 3] - np.asarray(AR.SCENE_LO)) / AR.SCENE_VOXEL
    a = np.floor(g).astype(np.int64)
    s = g - a
    t = tsdf.astype(np.float64)
    out = np.zeros(len(d))
    for i in (0, 1):
        for j in (0, 1):
            for k in (0, 1):
                wgt = (s[:, 0] if i else 1 - s[:, 0]) * (s[:, 1] if j else 1 - s[:, 1]) * (s[:, 2] if k else 1 - s[:, 2])
                out += wgt * t[a[:, 0] + i, a[:, 1] + j, a[:, 2] + k]
    return out, s


def test_jacobian_equals_central_differences_of_the_fp64_residual():
    """Perturbation as the step applies it: o + v, exp(omega) R (the retraction's first order).  The pose is 5 cm / 3
    degrees off the truth so that residuals and gradients are generic."""
    tsdf, weight, truth, depth = room(AR.PLANES_OFF)
    pose = AR.displaced(truth, 0.05, 3.0, np.random.default_rng(2))
    t = AR.pixel_terms(tsdf, weight, depth, pose, 1, AR.SCENE_INTR, AR.SCENE_LO, AR.SCENE_VOXEL)
    iv, iu = np.meshgrid(np.arange(AR.SCENE_H), np.arange(AR.SCENE_W), indexing="ij")
    iv, iu = iv.reshape(-1), iu.reshape(-1)
    f0, frac = residual64(tsdf, depth, pose, iu, iv)
    h = 1e-6                                      # metres and radians: a point moves by at most 3 h = 6e-5 cells
    inner = ((frac > 1e-3) & (frac < 1 - 1e-3)).all(1) & t["valid"]          # the differences must stay inside one cell
    assert inner.sum() > 2500
    fd = np.zeros((len(iu), 6))
    for i in range(6):
        e = np.zeros(6)
        e[i] = h
        plus = np.concatenate([AR.rotation(e[3:]) @ pose[:, :3], (pose[:, 3] + e[:3])[:, None]], 1)
        minus = np.concatenate([AR.rotation(-e[3:]) @ pose[:, :3], (pose[:, 3] - e[:3])[:, None]], 1)
        fd[:, i] = (residual64(tsdf, depth, plus, iu, iv)[0] - residual64(tsdf, depth, minus, iu, iv)[0]) / (2 * h)
    # Tolerance.  The restated gradient n is a difference of two doubly lerped corner values, all |.| <= 1: each of its
    # ~8 operations rounds by at most 2^-24, e_n = 8 * 2^-24.  Its sample point is computed in fp32 too: g has ~8
    # roundings of relative size 2^-24 at |g| <= 45 cells, dg = 8 * 2^-24 * 45 cells per axis, and the trilinear
    # gradient changes by at most the largest mixed second difference of a cell's corners per cell moved; corner values
    # of this room differ by at most voxel / trunc = 0.25 per step, which bounds that second difference.  So
    # |n - n_exact| <= e_n + 3 * dg * 0.25, gw = n / voxel, and the rotation entries q x gw carry |q| <= 3 m on each of
    # two products plus the fp32 rounding of q itself against |gw| <= 5 sqrt(3).  The central difference adds its own
    # fp64 rounding 2^-53 * |f| / h <= 1.2e-10 and no truncation error to speak of (the residual is cubic along a line:
    # h^2 / 6 * f''' ~ 1e-12).  The residual itself must agree to the lerp roundings plus the slope times dg.
    e_n = 8 * U32 + 3 * (8 * U32 * 45) * 0.25
    tol_t = e_n / AR.SCENE_VOXEL + 2e-10
    qmax = float(np.abs(t["q"][inner]).max())
    assert qmax <= 3.0
    tol_r = 2 * qmax * tol_t + 2 * (4 * U32 * qmax) * 5 * math.sqrt(3) + 2e-10
    J = t["J"].astype(np.float64)
    err_t = np.abs(J[inner, :3] - fd[inner, :3]).max()
    err_r = np.abs(J[inner, 3:] - fd[inner, 3:]).max()
    err_f = np.abs(t["f"][inner].astype(np.float64) - f0[inner]).max()
    print(f"{inner.sum()} samples: |J - fd| translation {err_t:.3e} (tol {tol_t:.3e}), rotation {err_r:.3e} (tol {tol_r:.3e}), "
          f"|f - f64| {err_f:.3e}; largest |J| {np.abs(J[inner]).max():.3f}")
    assert np.abs(fd[inner]).max() > 1.0                        # the comparison is not between zeros
    assert err_t <= tol_t and err_r <= tol_r
    assert err_f <= 8 * U32 + 3 * (8 * U32 * 45) * 0.25


def test_sums_equal_a_plain_fp64_normal_system():
    """H, b, cost and sq against np.einsum over the same fp32 J, wt and f, within n * 2^-52 relative per entry: of the
    entry itself, mixed signs or not.  (Two summation orders of n terms differ by at most n * 2^-52 of the sum of the
    terms' magnitudes; that weaker statement is asserted as well, and printed is how far the entries stay below the
    stronger one.)"""
    tsdf, weight, truth, depth = room(AR.PLANES_OFF)
    pose = AR.displaced(truth, 0.08, 4.0, np.random.default_rng(4))
    for stride, huber in ((1, 0.5), (2, 0.05), (3, 0.5)):
        t = AR.pixel_terms(tsdf, weight, depth, pose, stride, AR.SCENE_INTR, AR.SCENE_LO, AR.SCENE_VOXEL, huber=huber)
        row = AR.system(tsdf, weight, depth[None], [0], pose[None], stride, AR.SCENE_INTR, AR.SCENE_LO, AR.SCENE_VOXEL, CHUNK,
                        huber=huber)[0]
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
            assert abs(row[21 + i] - bi) <= n * 2.0 ** -52 * (w * np.abs(J[:, i] * f)).sum()
            worst = max(worst, abs(row[21 + i] - bi) / (n * 2.0 ** -52 * abs(bi)))
        print(f"stride {stride}, huber {huber}: n = {n}, largest error {worst:.4f} of n 2^-52 |entry|")
        assert abs(row[27] - (w * f * f).sum()) <= n * 2.0 ** -52 * row[27]
        assert abs(row[29] - (f * f).sum()) <= n * 2.0 ** -52 * row[29]


# ---- the retraction -------------------------------------------------------------------------------------------------
def hundred_steps(seed, size):
    """|R^T R - I| (largest entry), det R and the translation's error after 100 steps of about `size` from a generic pose."""
    rng = np.random.default_rng(seed)
    m = np.concatenate([AR.rotation(rng.normal(size=3)), np.zeros((3, 1))], 1).tolist()
    o = np.zeros(3)
    for _ in range(100):
        x = rng.normal(size=6) * size
        m = AR.retract(m, [float(v) for v in x])
        o += x[:3]
    R = np.array(m)[:, :3]
    return np.abs(R.T @ R - np.eye(3)).max(), np.linalg.det(R), np.abs(np.array(m)[:, 3] - o).max()


def test_retraction_stays_a_rotation_to_1e_15_after_100_steps():
    """|R^T R - I| <= 1e-15 after 100 steps, for steps of every size.  The product dR R alone does not give this: its
    roundings add up to 5e-15 in the median and 1.2e-14 at most over these 20 starts (3e-14 for steps of 1e-6).  The
    step's Newton correction R = P (I - E / 2), E = P^T P - I, removes what the step before left, so the departure is
    that of one step: measured at most 4.4e-16 at any of the 100 steps."""
    for size in (0.3, 0.05, 1e-3, 1e-6):
        devs = [hundred_steps(seed, size) for seed in range(20)]
        worst = max(d[0] for d in devs)
        print("step size", size, "largest |R^T R - I| after 100 steps over 20 seeds:", worst)
        assert worst <= 1e-15 and all(d[1] > 0.999 for d in devs)
        assert all(d[2] <= 100 * 2.0 ** -52 * 100 * size * 4 + 1e-300 for d in devs)     # the translation is a plain sum


def test_the_correction_is_needed_and_moves_a_rotation_by_roundings_only():
    """Without the Newton step the same 100 products leave the rotations by more than the bound (so the test above does
    test it), and the step changes a rotation matrix by no more than its own departure |E| / 2 plus roundings."""
    rng = np.random.default_rng(0)
    R = AR.rotation(rng.normal(size=3))
    plain = R.copy()
    m = np.concatenate([R, np.zeros((3, 1))], 1).tolist()
    for _ in range(100):
        w = rng.normal(size=3) * 0.05
        before = np.array(m)[:, :3]
        m = AR.retract(m, [0.0, 0.0, 0.0] + [float(v) for v in w])
        h = w / 2
        q = np.concatenate([[1.0], h]) / math.sqrt(1 + h @ h)
        a, b, c, d = q
        dR = np.array([[a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)],
                       [2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b)],
                       [2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d]])
        assert np.abs(np.array(m)[:, :3] - dR @ before).max() <= 8 * 2.0 ** -52
        plain = dR @ plain
    drift = np.abs(plain.T @ plain - np.eye(3)).max()
    print("|R^T R - I| of the uncorrected product:", drift)
    assert drift > 1e-15


def test_retraction_agrees_with_exp_to_second_order():
    # the unit quaternion (1, w / 2) / |.| turns by 2 atan(|w| / 2) = |w| - |w|^3 / 12 + ... about w: exp's axis, and its
    # angle up to the third order.  |R(a) - R(b)|_F = 2 sqrt(2) sin(|a - b| / 2) about a common axis.
    axis = np.array([0.36, -0.48, 0.8])
    eye = np.concatenate([np.eye(3), np.zeros((3, 1))], 1).tolist()
    for angle in (0.2, 0.02, 0.002):
        w = axis * angle
        got = np.array(AR.retract(eye, [0.0, 0.0, 0.0] + [float(v) for v in w]))[:, :3]
        diff = np.linalg.norm(got - AR.rotation(w))
        want = 2 * math.sqrt(2) * math.sin((angle - 2 * math.atan(angle / 2)) / 2)
        print(f"|w| = {angle}: |retract - exp|_F = {diff:.3e}, third-order term {want:.3e}")
        assert abs(diff - want) <= 1e-15 + 1e-12 * want
        assert want <= math.sqrt(2) * angle ** 3 / 12 * 1.001


# ---- convergence ----------------------------------------------------------------------------------------------------
def run_starts(planes, seed):
    tsdf, weight, truth, depth = room(planes)
    rng = np.random.default_rng(seed)
    starts = np.stack([AR.displaced(truth, 0.05, 3.0, rng) for _ in range(20)] +
                      [AR.displaced(truth, 0.10, 5.0, rng) for _ in range(10)])
    pose, rows, trace = AR.align(tsdf, weight, depth[None], [0] * 30, starts, AR.SCENE_INTR, AR.SCENE_LO, AR.SCENE_VOXEL, CHUNK)
    return truth, starts, pose, rows, trace


def test_every_start_returns_to_the_truth_with_planes_on_the_lattice():
    """20 starts at 5 cm / 3 degrees and 10 at 10 cm / 5 degrees, default levels.  On lattice planes the interpolant is
    exact at the surface, so only fp32 rounding keeps the fixed point from the truth."""
    truth, starts, pose, rows, trace = run_starts(AR.PLANES_ON, 21)
    errs = np.array([AR.pose_error(p, truth) for p in pose])
    print("largest error:", errs[:, 0].max(), "m,", errs[:, 1].max(), "deg; cost", rows[:, 27].max())
    assert trace.shape == (25, 30, 4) and (trace[:, :, 3] == 1).all() and (rows[:, 28] == 3072).all()
    assert errs[:, 0].max() <= AR.SCENE_VOXEL / 100 and errs[:, 1].max() <= 0.01


def test_every_start_ends_at_one_point_with_planes_off_the_lattice():
    """The fixed point is off the truth by the bias of the cells that straddle a crease: measured with this restatement
    (fp32 gather, fp64 sums) 0.758 mm and 0.0155 degrees, all 30 starts within 1e-7 m of one another."""
    truth, starts, pose, rows, trace = run_starts(AR.PLANES_OFF, 22)
    errs = np.array([AR.pose_error(p, truth) for p in pose])
    pairs = np.array([AR.pose_error(p, q) for i, p in enumerate(pose) for q in pose[i + 1:]])
    spread, turn = pairs[:, 0].max(), pairs[:, 1].max()
    print("error:", errs[:, 0].min(), "..", errs[:, 0].max(), "m,", errs[:, 1].min(), "..", errs[:, 1].max(),
          "deg; largest distance between two ends", spread, "m,", turn, "deg")
    assert (trace[:, :, 3] == 1).all()
    assert spread <= 1e-5                                       # every pair of the 30, not only against the first
    # two ends that differ by an angle t about the camera centre put the surface points, all further than 0.9 m away, more
    # than 0.9 t apart: ends that agree to 1e-5 m in what they explain agree to 1e-5 / 0.9 rad
    assert turn <= math.degrees(1e-5 / 0.9)
    assert errs[:, 0].max() <= AR.SCENE_VOXEL / 10 and errs[:, 1].max() <= 0.1


def test_a_start_at_the_truncation_distance_runs_to_the_end():
    """20 cm / 10 degrees equals the truncation: where it ends is not asserted, only that every step reports itself."""
    tsdf, weight, truth, depth = room(AR.PLANES_ON)
    start = AR.displaced(truth, 0.20, 10.0, np.random.default_rng(23))
    pose, rows, trace = AR.align(tsdf, weight, depth[None], [0], start[None], AR.SCENE_INTR, AR.SCENE_LO, AR.SCENE_VOXEL, CHUNK)
    print("ends", AR.pose_error(pose[0], truth), "from the truth; status", trace[:, 0, 3])
    assert np.isfinite(pose).all() and set(trace[:, 0, 3]) <= {0.0, 1.0}


# ---- the contract's corners -----------------------------------------------------------------------------------------
def test_an_image_of_zeros_leaves_the_pose_alone():
    tsdf, weight, truth, depth = room(AR.PLANES_ON)
    pose, rows, trace = AR.align(tsdf, weight, np.zeros_like(depth)[None], [0], truth[None], AR.SCENE_INTR, AR.SCENE_LO,
                                 AR.SCENE_VOXEL, CHUNK)
    assert not rows.any() and not trace.any() and np.array_equal(pose[0], truth)


def test_a_single_plane_fails_its_pivot_without_lam_abs():
    """A wall seen head-on constrains z and two rotations: H's first pivot is 0, and lam_rel * 0 does not help."""
    dims, voxel = (17, 17, 17), 0.125
    z = voxel * np.arange(17)
    tsdf = np.broadcast_to(np.clip((1.5 - z) / 0.5, -1, 1).astype(np.float32), dims).copy()
    weight = np.ones(dims, np.float32)
    depth = np.full((1, 16, 16), 1.25, np.float32)
    pose = np.array([[1.0, 0, 0, 1.0], [0, 1.0, 0, 1.0], [0, 0, 1.0, 0.1]])
    intr = (40.0, 40.0, 7.5, 7.5)
    rows = AR.system(tsdf, weight, depth, [0], pose[None], 1, intr, (0, 0, 0), voxel, CHUNK)
    assert rows[0, 28] == 256 and rows[0, 0] == 0 and rows[0, 11] > 0          # H_00 = 0, H_22 > 0
    moved, trace = AR.step(rows, pose[None], lam_rel=1e-6, lam_abs=0.0, min_count=64)
    assert trace[0, 3] == 0 and trace[0, 1] == 256 and np.array_equal(moved[0], pose)
    moved, trace = AR.step(rows, pose[None], lam_rel=1e-6, lam_abs=1e-9, min_count=64)
    assert trace[0, 3] == 1 and abs(moved[0, 2, 3] - 0.25) < 1e-6              # one step lands on the wall: 1.5 - 1.25
    assert np.array_equal(moved[0, :2, 3], pose[:2, 3])                        # nothing pushes along the wall
    moved, trace = AR.step(rows, pose[None], min_count=257)
    assert trace[0, 3] == 0 and np.array_equal(moved[0], pose)


def constant_field(value):
    dims = (5, 5, 5)
    return np.full(dims, value, np.float32), np.ones(dims, np.float32)


def one_pixel(tsdf, weight, point, depth=1.0, **kw):
    """One pixel on the optical axis of an identity camera at point - (0, 0, depth), lattice lo = 0, voxel = 0.125."""
    pose = np.concatenate([np.eye(3), (np.asarray(point, np.float64) - [0, 0, depth])[:, None]], 1)
    return AR.system(tsdf, weight, np.full((1, 1, 1), depth, np.float32), [0], pose[None], 1, (1.0, 1.0, 0.0, 0.0),
                     (0, 0, 0), 0.125, CHUNK, **kw)[0]


def test_huber_weight_at_the_threshold_and_the_saturation_test():
    tsdf, weight = constant_field(0.5)
    at = one_pixel(tsdf, weight, (0.3, 0.3, 0.3), huber=0.5)
    assert at[28] == 1 and at[27] == 0.25 and at[29] == 0.25                   # |f| == huber: weight 1
    below = one_pixel(tsdf, weight, (0.3, 0.3, 0.3), huber=0.25)
    assert below[27] == 0.125 and below[29] == 0.25                            # weight huber / |f| = 0.5
    assert one_pixel(*constant_field(1.0), (0.3, 0.3, 0.3))[28] == 0           # |f| < 1 fails at 1
    assert one_pixel(*constant_field(-1.0), (0.3, 0.3, 0.3))[28] == 0
    assert one_pixel(*constant_field(np.float32(1.0) - np.float32(2.0 ** -24)), (0.3, 0.3, 0.3))[28] == 1


def test_max_depth_keeps_the_pixel_considered():
    tsdf, weight = constant_field(0.25)
    assert one_pixel(tsdf, weight, (0.3, 0.3, 0.3), depth=1.0, max_depth=1.0)[[28, 30]].tolist() == [1, 1]
    assert one_pixel(tsdf, weight, (0.3, 0.3, 0.3), depth=1.0, max_depth=0.999)[[28, 30]].tolist() == [0, 1]
    for bad in (0.0, -1.0, math.nan):
        assert one_pixel(tsdf, weight, (0.3, 0.3, 0.3), depth=bad)[[28, 30]].tolist() == [0, 0]


def test_the_last_cell_is_valid_and_the_far_face_is_not():
    """5 points per axis at voxel 0.125: cells 0 .. 3, the far face at 0.5."""
    tsdf, weight = constant_field(0.25)
    assert one_pixel(tsdf, weight, (0.4375, 0.4375, 0.4375))[28] == 1          # g = 3.5 on every axis
    assert one_pixel(tsdf, weight, (0.0, 0.0, 0.0))[28] == 1                    # g = 0: the first cell
    for axis in range(3):
        p = [0.25, 0.25, 0.25]
        p[axis] = 0.5
        assert one_pixel(tsdf, weight, p)[[28, 30]].tolist() == [0, 1]         # floor(g) = 4 = n - 1
        p[axis] = -0.0078125
        assert one_pixel(tsdf, weight, p)[28] == 0
    weight[4, 4, 4] = 0.0
    assert one_pixel(tsdf, weight, (0.4375, 0.4375, 0.4375))[28] == 0           # one corner unseen
    assert one_pixel(tsdf, weight, (0.4375, 0.4375, 0.4375), min_weight=0.0)[28] == 1


# ---- go_slam_amd/localize.py on the host ----------------------------------------------------------------------------
@pytest.fixture()
def no_library(monkeypatch):
    from go_slam_amd import _lib

    def refuse():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "lib", refuse)


def test_every_host_side_refusal(no_library):
    from go_slam_amd import localize
    vol = types.SimpleNamespace(device=torch.device("cpu"), dims=(5, 5, 5), lo=np.zeros(3), voxel=0.1, trunc=0.4)
    depth = torch.ones(2, 4, 6)
    eye = np.eye(4)[None].repeat(2, 0)
    intr = (5.0, 5.0, 2.5, 1.5)
    bad_align = [
        dict(depth=torch.ones(4)), dict(depth=torch.ones(2, 0, 6)), dict(depth=torch.ones(1, 2, 4, 6)),
        dict(c2w_init=np.eye(4)[None].repeat(3, 0)), dict(c2w_init=np.zeros((2, 4, 3))), dict(c2w_init=eye * math.nan),
        dict(intrinsics=(1.0, 1.0, 0.0)), dict(intrinsics=(0.0, 5.0, 2.5, 1.5)), dict(intrinsics=(5.0, 0.0, 2.5, 1.5)),
        dict(intrinsics=(5.0, 5.0, math.inf, 1.5)),
        dict(frame=[0]), dict(frame=[0, 2]), dict(frame=[-1, 0]), dict(frame=[0.0, 1.0]), dict(frame=[[0, 1]]),
        dict(levels=()), dict(levels=((0, 5),)), dict(levels=((2, -1),)), dict(levels=((1.5, 2),)), dict(levels=(4, 10)),
        dict(huber=0.0), dict(huber=-0.5), dict(huber=math.nan), dict(max_depth=0.0), dict(max_depth=math.nan),
        dict(min_weight=math.nan), dict(lam_rel=-1e-6), dict(lam_rel=math.inf), dict(lam_abs=math.nan), dict(lam_abs=-1.0),
        dict(min_count=0), dict(min_count=2.5), dict(min_count=True)]
    for bad in bad_align:
        args = dict(dict(depth=depth, c2w_init=eye, intrinsics=intr), **bad)
        with pytest.raises(ValueError, match="TSDFVolume.align"):
            localize.align(vol, **args)
    for bad in (dict(stride=0), dict(stride=1.5), dict(stride=True), dict(huber=0.0), dict(frame=[0, 5]),
                dict(c2w=np.zeros((2, 2, 2)))):
        args = dict(dict(depth=depth, c2w=eye, intrinsics=intr), **bad)
        with pytest.raises(ValueError, match="TSDFVolume.pose_scores"):
            localize.pose_scores(vol, **args)
    for bad in (dict(depth=depth), dict(keep=0), dict(keep=1.5), dict(min_inlier_fraction=math.nan),
                dict(candidates=np.zeros((3, 2, 2)))):
        args = dict(dict(depth=depth[0], intrinsics=intr, candidates=eye), **bad)
        with pytest.raises(ValueError, match="relocalize"):
            localize.relocalize(vol, **args)
    assert localize.relocalize(vol, depth[0], intr, np.zeros((0, 4, 4)))["found"] is False
    for bad in (dict(centres=[[0, 0]]), dict(centres=[[0, 0, math.nan]]), dict(n_yaw=0), dict(n_yaw=2.5), dict(up_axis=3),
                dict(up_axis=True), dict(pitch=math.inf), dict(up_sign=0)):
        args = dict(dict(centres=[[0.0, 0.0, 0.0]], n_yaw=4, up_axis=2), **bad)
        with pytest.raises(ValueError, match="candidate_poses"):
            localize.candidate_poses(**args)
    with pytest.raises(ValueError, match="every"):
        localize.align_stream(vol, [], [], intr, every=0)


def test_candidate_poses_follow_ray_directions_headings():
    """A candidate's optical axis is the central ray of view.ray_directions at the same yaw and pitch, for every up
    axis; the frame is right-handed with the image's y against the up axis."""
    from go_slam_amd import localize, view
    centres = np.array([[0.5, -1.0, 2.0], [3.0, 0.25, -0.75]])
    for up in (0, 1, 2):
        for sign in (1, -1):
            c = localize.candidate_poses(centres, 8, up, pitch=0.2, up_sign=sign)
            assert c.shape == (16, 4, 4) and np.array_equal(c[:, 3], np.tile([0, 0, 0, 1.0], (16, 1)))
            assert np.array_equal(c[:8, :3, 3], np.tile(centres[0], (8, 1))) and np.array_equal(c[8:, :3, 3],
                                                                                              np.tile(centres[1], (8, 1)))
            R = c[:, :3, :3]
            assert np.abs(R.transpose(0, 2, 1) @ R - np.eye(3)).max() <= 1e-15
            assert np.allclose(np.linalg.det(R), 1.0, rtol=0, atol=1e-15)
            assert (sign * R[:, up, 1] < 0).all()                # image y against up
            assert np.abs(R[:, up, 0]).max() <= 1e-16            # no roll
            for j in range(8):
                ray = view.ray_directions(60.0, 45.0, 1, 1, 2 * math.pi * j / 8, sign * 0.2, up)[0].astype(np.float64)
                ray /= np.linalg.norm(ray)
                assert np.abs(ray - R[j, :, 2]).max() <= 1.5 / view.MAX_DIR      # the integer ray's own rounding


def fake_volume(seed=0):
    from go_slam_amd.tsdf import TSDFVolume
    g = torch.Generator().manual_seed(seed)
    vol = TSDFVolume.__new__(TSDFVolume)
    vol.voxel, vol.lo, vol.dims, vol.trunc, vol.max_weight = 0.07, np.array([-0.3, 0.1, 1e-17]), (4, 3, 5), 0.3, 17.0
    vol.device = torch.device("cpu")
    vol.tsdf = torch.rand(4, 3, 5, generator=g) * 2 - 1
    vol.weight = torch.rand(4, 3, 5, generator=g) * 9
    vol.colors = torch.rand(3, 4, 3, 5, generator=g)
    vol._flags = None
    return vol


def test_save_and_load_round_trip_bit_for_bit(tmp_path):
    from go_slam_amd.tsdf import TSDFVolume
    vol = fake_volume()
    vol.tsdf[0, 0, 0], vol.tsdf[1, 1, 1] = -0.0, float(np.float32(1e-45))       # a signed zero and a denormal survive
    path = str(tmp_path / "vol.npz")
    vol.save(path)
    back = TSDFVolume.load(path, device="cpu")
    assert isinstance(back, TSDFVolume) and back.dims == vol.dims and back._flags is None
    assert (back.voxel, back.trunc, back.max_weight) == (vol.voxel, vol.trunc, vol.max_weight)
    assert np.array_equal(back.lo.view(np.int64), vol.lo.view(np.int64))
    for a, b in ((back.tsdf, vol.tsdf), (back.weight, vol.weight), (back.colors, vol.colors)):
        assert a.dtype == torch.float32 and np.array_equal(a.numpy().view(np.int32), b.numpy().view(np.int32))
    data = dict(np.load(path))
    assert sorted(data) == sorted(("tsdf", "weight", "colors", "lo", "voxel", "trunc", "max_weight", "dims"))
    for bad in (dict(dims=np.array([4, 3, 6])), dict(dims=np.array([4, 3])), dict(dims=np.array([1, 3, 5])),
                dict(weight=data["weight"][:3]), dict(colors=data["colors"][:2]), dict(tsdf=data["tsdf"].astype(np.float64)),
                dict(voxel=np.float64(0.0)), dict(trunc=np.float64(math.nan)), dict(max_weight=np.float64(0.5)),
                dict(lo=np.array([0.0, math.inf, 0.0]))):
        other = str(tmp_path / "bad.npz")
        np.savez(other, **dict(data, **bad))
        with pytest.raises(ValueError, match="TSDFVolume.load"):
            TSDFVolume.load(other, device="cpu")
    del data["trunc"]
    np.savez(str(tmp_path / "short.npz"), **data)
    with pytest.raises(ValueError, match="lacks"):
        TSDFVolume.load(str(tmp_path / "short.npz"), device="cpu")


def test_align_text_round_trip_bit_for_bit():
    from go_slam_amd import localize
    per_frame = np.array([[0.1, 1 / 3, 2.0 ** -40, 0.7, 0.05, 3.0, 1.0], [1e-300, 179.99999999999997, 5e-324, 1.0, 0.0, 2.0, 1.0],
                          [0.0, 0.0, math.inf, 0.0, 0.0, 0.0, 0.0], [0.30000000000000004, 2.5, 0.011, 0.5, 0.1, 3.0, 1.0]])
    frames = [0, 5, 10, 15]
    result = localize.summarize_align(per_frame)
    assert result["n_failed"] == 1 and result["n_frames"] == 4 and result["moved_max_m"] == 0.30000000000000004
    assert result["inlier_fraction_min"] == 0.5 and result["rmse_max_m"] == 0.011
    assert result["n_underconstrained"] == 1 and result["moved_constrained_max_m"] == 0.1
    assert result["moved_constrained_mean_m"] == (0.05 + 0.0 + 0.1) / 3
    text = localize.align_text(result, frames, per_frame)
    back, rows = localize.parse_align(text)
    assert list(back) == list(localize.ALIGN_REPORT_ORDER)
    assert all(np.float64(back[k]).view(np.int64) == np.float64(result[k]).view(np.int64) for k in back)
    assert [r[0] for r in rows] == frames
    assert np.array_equal(np.array([r[1:] for r in rows], np.float64).view(np.int64), per_frame.view(np.int64))
    empty = localize.summarize_align(np.zeros((0, 7)))
    assert math.isnan(empty["moved_mean_m"]) and empty["n_frames"] == 0 and empty["n_underconstrained"] == 0
    back, rows = localize.parse_align(localize.align_text(empty, [], np.zeros((0, 7))))
    assert math.isnan(back["rmse_max_m"]) and rows == []
    with pytest.raises(ValueError):
        localize.parse_align("something else\n")


def rows_of(normals, weights):
    """A system row whose translation block is sum w n n^T."""
    row = np.zeros(32)
    H = sum(w * np.outer(n, n) for n, w in zip(np.asarray(normals, np.float64), weights))
    row[[0, 1, 2, 6, 7, 11]] = H[0, 0], H[0, 1], H[0, 2], H[1, 1], H[1, 2], H[2, 2]
    return row


def test_constrained_movement_drops_the_free_directions():
    """A wall z and a floor y leave x free; three planes leave nothing free; a plane seen by fewer than a hundredth of
    the samples does not count; a rotated pair frees the rotated edge."""
    from go_slam_amd import localize
    moved = np.array([1.3, 0.003, -0.004])
    two = rows_of([[0, 0, 1], [0, 1, 0]], [2000, 1000])
    two[0] = 3.0                                              # what noise leaves on the free axis: 1.5e-3 of the largest
    three = rows_of([[0, 0, 1], [0, 1, 0], [1, 0, 0]], [2000, 1000, 500])
    sliver = rows_of([[0, 0, 1], [0, 1, 0], [1, 0, 0]], [2000, 1000, 19])
    c, s = math.cos(0.3), math.sin(0.3)
    turned = rows_of([[s, 0, c], [0, 1, 0]], [2000, 1000])    # the free edge is (c, 0, -s)
    rows = np.stack([two, three, sliver, turned, np.zeros(32)])
    m, n = localize.constrained_movement(rows, np.tile(moved, (5, 1)))
    assert n.tolist() == [2, 3, 2, 2, 0]
    assert abs(m[0] - 0.005) <= 1e-15 and abs(m[2] - 0.005) <= 1e-15 and m[4] == 0
    assert abs(m[1] - np.linalg.norm(moved)) <= 1e-15
    edge = np.array([c, 0, -s])
    assert abs(m[3] - np.linalg.norm(moved - (moved @ edge) * edge)) <= 1e-15
    assert localize.CONSTRAINED_SHARE == 0.01


def test_align_key_is_refused_before_anything_is_fused(tmp_path):
    """tsdf.align in a mode without sensor depth, or without the stream, raises before the video is touched: the
    namespace has no video, no output directory is written."""
    from go_slam_amd.tsdf import fuse_from_config
    cfg = {"mode": "mono", "mapping": {"bound": [[0, 1], [0, 1], [0, 1]]},
           "tsdf": {"enable": True, "align": {"enable": True}}}
    slam = types.SimpleNamespace(cfg=cfg, output=str(tmp_path / "out"), mode="mono")
    with pytest.raises(ValueError, match="tsdf.align needs rgbd mode"):
        fuse_from_config(slam, stream=[], c2w_list=[])
    cfg["mode"] = "rgbd"
    with pytest.raises(ValueError, match="tsdf.align needs the stream"):
        fuse_from_config(slam, stream=None, c2w_list=[])
    with pytest.raises(ValueError, match="tsdf.align needs the stream"):
        fuse_from_config(slam, stream=[], c2w_list=None)
    assert not os.path.exists(slam.output)
    cfg["tsdf"]["align"]["enable"] = False
    with pytest.raises(AttributeError):                         # without the key it goes on to the video, as before
        fuse_from_config(slam, stream=None, c2w_list=None)


def test_workspace_size_needs_no_gpu(built_lib):
    from go_slam_amd import _lib
    L = _lib.lib()
    C = L.gs_tsdf_align_chunk()
    assert C in (1024, 2048, 4096)
    assert L.gs_tsdf_align_workspace_bytes(1, 1, 1, 1) == 256
    assert L.gs_tsdf_align_workspace_bytes(3, 480, 640, 1) == 3 * (480 * 640 // C) * 256
    assert L.gs_tsdf_align_workspace_bytes(3, 480, 640, 4) == 3 * -(-(120 * 160) // C) * 256
    assert L.gs_tsdf_align_workspace_bytes(2, 7, 9, 5) == 2 * 256                         # ceil(7/5) * ceil(9/5) = 4 samples
    for bad in ((-1, 4, 4, 1), (1, 0, 4, 1), (1, 4, 0, 1), (1, 4, 4, 0), (1, 1 << 16, 1 << 15, 1), (1 << 30, 480, 640, 1)):
        assert L.gs_tsdf_align_workspace_bytes(*bad) == 0, bad


# ---- the kernel's budget (compile only, as tests/test_abi.py does for its kernels) ------------------------------------
def test_align_kernels_fit_their_budget(tmp_path):
    """tsdf_align_system_kernel is a gather with 29 fp64 accumulators: four waves per SIMD need at most 128 VGPRs, and a
    spilled accumulator would turn every sample into scratch traffic.  Its only LDS is the four waves' rows, 4 x 32
    doubles.  The two small kernels use no LDS and no scratch."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "go_slam_amd", "csrc")
    out = tmp_path / "k.s"
    res = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-gpu-rdc",
                          "-munsafe-fp-atomics", "-I", csrc, "-I", os.path.join(ROOT, "include"), "--cuda-device-only", "-S",
                          os.path.join(csrc, "tsdf_align.hip"), "-o", str(out)],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-2000:]
    assert "failed to meet occupancy target" not in res.stdout, res.stdout[-2000:]
    pat = re.compile(r"\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.name:\s+(\S+)\n(?:.*\n)*?"
                     r"\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)")
    budgets = {"tsdf_align_system_kernel": (128, 4 * 32 * 8), "tsdf_align_sum_kernel": (128, 0),
               "tsdf_align_step_kernel": (128, 0)}
    seen = set()
    for m in pat.finditer(open(out).read()):
        lds, name, scratch, vgpr = int(m.group(1)), m.group(2), int(m.group(3)), int(m.group(4))
        for key, (max_vgpr, max_lds) in budgets.items():
            if key in name:
                seen.add(key)
                print(name, "VGPRs", vgpr, "LDS", lds, "scratch", scratch)
                assert scratch == 0 and vgpr <= max_vgpr and lds <= max_lds, (name, scratch, vgpr, lds)
    assert seen == set(budgets)
