"""The raycast contract (include/goslam_hip.h, gs_tsdf_raycast) on the CPU: tests/tsdf_raycast_restatement.py against
closed forms (a plane, a sphere), the edge cases of the march with their expected results spelled out, the brick skip
against the plain march, and the Python surface that needs no launch."""
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import tsdf_raycast_restatement as RR                          # noqa: E402
import tsdf_restatement as TR                                  # noqa: E402

EPS = 2.0 ** -24                                               # half an ulp of 1 in fp32
HW = TR.PLANE_HW
INTR = tuple(float(np.float32(v)) for v in TR.PLANE_INTR)      # rounded once, for the same reason as look()'s matrix


def look(yaw_deg, pitch_deg, centre):
    """[3,4] camera-to-world matrix of a camera turned by yaw about y, then pitch about its x, rounded to fp32."""
    a, b = math.radians(yaw_deg), math.radians(pitch_deg)
    Ry = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
    Rx = np.array([[1, 0, 0], [0, math.cos(b), -math.sin(b)], [0, math.sin(b), math.cos(b)]])
    m = np.concatenate([Ry @ Rx, np.asarray(centre, np.float64)[:, None]], 1)
    return m.astype(np.float32).astype(np.float64)             # what every precision of the march is given


def rays(c2w, intr, size):
    """float64 world directions [H,W,3] of the pixel rays (dx, dy, 1) and the camera centre."""
    fx, fy, cx, cy = intr
    m = np.asarray(c2w, np.float64)
    v, u = np.meshgrid(np.arange(size[0], dtype=np.float64), np.arange(size[1], dtype=np.float64), indexing="ij")
    d = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1)
    return d @ m[:, :3].T, m[:, 3]


# ---- plane ----------------------------------------------------------------------------------------------------------
PLANE_C = 2.03125                       # exact in fp32, as are the depths of the two cameras with centre z = 0
PLANE_VIEW = look(14.0, -9.0, (0.15, -0.1, 0.25))
# fp32 against fp64 on the plane: the march is a few dozen fp32 operations on t (<= 2.5 m) and on index coordinates
# g (g * voxel <= 2.5 m), each rounding at most 2^-24 of its magnitude; the crossing moves by the sum of those
# divided by the ray's z-slope (>= 1/2 for this view).  32 roundings * 2^-24 * 2.5 m * 2 = 9.6e-6 m.
PLANE_FP32_BOUND = 32 * EPS * 2.5 * 2
# normals: a component is a difference of trilinear values f (|f| <= 1/2 this close to the surface) over one cell, where
# the field changes by voxel / trunc = 1/4: 8 roundings * 2^-24 * (1/2) / (1/4) = 9.6e-7 per component before normalising
PLANE_NORMAL_BOUND = 8 * EPS * 0.5 / 0.25


@pytest.fixture(scope="module")
def plane_case():
    """The lattices of TR.plane_scene's first two cameras (the ones with exact depth) in fp64 and fp32, and their
    raycasts from an oblique pose."""
    depth, w2c = TR.plane_scene(PLANE_C)
    depth, w2c = depth[:2], w2c[:2]
    assert (depth.astype(np.float64) == PLANE_C).all()
    dims = TR.lattice_dims(TR.PLANE_BOUND, TR.PLANE_VOXEL)
    lo = TR.PLANE_BOUND[:, 0]
    out = {}
    for T in (np.float64, np.float32):
        vol = TR.integrate(TR.new_volume(dims, T), depth, w2c, TR.PLANE_INTR, lo, TR.PLANE_VOXEL, 4 * TR.PLANE_VOXEL,
                           dtype=T)
        out[T] = (vol, RR.raycast(vol, PLANE_VIEW[None], INTR, HW, lo, TR.PLANE_VOXEL, dtype=T))
    return out


def plane_truth():
    dw, o = rays(PLANE_VIEW, INTR, HW)
    return (PLANE_C - o[2]) / dw[..., 2]


def test_plane_depth_fp64_is_analytic_and_fp32_within_its_roundings(plane_case):
    """In fp64 the lattice is linear in z up to 1e-15, trilinear interpolation and the secant step are exact for a
    linear field: what remains is rounding, far below 1e-9 m."""
    truth = plane_truth()
    d64, d32 = plane_case[np.float64][1]["depth"][0], plane_case[np.float32][1]["depth"][0]
    hit = d64 > 0
    assert hit.mean() > 0.5 and np.array_equal(hit, d32 > 0)
    e64 = np.abs(d64 - truth)[hit].max()
    e32 = np.abs(d32.astype(np.float64) - truth)[hit].max()
    print(f"plane: {hit.sum()} hits, fp64 error {e64:.3e} m, fp32 error {e32:.3e} m (bound {PLANE_FP32_BOUND:.3e})")
    assert e64 <= 1e-9
    assert e32 <= e64 + PLANE_FP32_BOUND


def test_plane_normals_point_at_the_cameras(plane_case):
    for T, bound in ((np.float64, 1e-9), (np.float32, PLANE_NORMAL_BOUND)):
        out = plane_case[T][1]
        hit = out["depth"][0] > 0
        n = out["normal"][0][hit].astype(np.float64)
        err = np.abs(n - np.array([0.0, 0.0, -1.0])).max()
        print(f"plane normals {T.__name__}: largest component error {err:.3e} (bound {bound:.3e})")
        assert err <= bound
        assert not out["normal"][0][~hit].any()


# ---- sphere ---------------------------------------------------------------------------------------------------------
SPH_R, SPH_C, SPH_H = 0.8, np.array([0.05, -0.02, 0.03]), 0.05
SPH_LO, SPH_N = np.array([-1.2, -1.2, -1.2]), 49
SPH_STEP = 0.5


@pytest.fixture(scope="module")
def sphere_volume():
    ax = [SPH_LO[a] + np.arange(SPH_N) * SPH_H for a in range(3)]
    p = np.stack(np.meshgrid(*ax, indexing="ij"), -1)
    tsdf = np.clip((np.linalg.norm(p - SPH_C, axis=-1) - SPH_R) / (4 * SPH_H), -1.0, 1.0)
    rgb = np.stack([0.5 + 0.5 * np.sin(3.0 * p[..., c]) for c in range(3)])
    return {"tsdf": tsdf, "weight": np.ones_like(tsdf), "colors": rgb}


SPH_VIEW = look(6.0, -4.0, (0.3, -0.2, -3.0))


def test_sphere_depth_within_the_interpolation_and_step_bound(sphere_volume):
    """phi = |p - c| - r has second derivatives summing to 2 / rho.  Trilinear interpolation on cells of side h is off by
    at most (h^2 / 8) * that sum = h^2 / (4 rho).  Along a ray |phi''| <= 1 / rho, so the chord between two samples
    delta = step * h apart is off by at most delta^2 / (8 rho).  The crossing of the chord through two interpolated
    samples therefore lies where |phi| <= h^2 / (4 rho) + delta^2 / (8 rho); phi changes along the ray at the incidence
    cosine, >= 0.5 at the analytic hit and by at most delta / rho less over one step.  rho >= r - 2h wherever a sample
    next to the surface lies; nothing within h + delta < trunc = 4h of the surface is clamped.  The ray parameter t
    advances |dw| >= 1 metres per unit, so the bound in metres also bounds t."""
    h, delta, rho = SPH_H, SPH_STEP * SPH_H, SPH_R - 2 * SPH_H
    bound = (h * h / (4 * rho) + delta * delta / (8 * rho)) / (0.5 - delta / rho)
    dw, o = rays(SPH_VIEW, INTR, HW)
    a = (dw * dw).sum(-1)
    b = (dw * (o - SPH_C)).sum(-1)
    disc = b * b - a * (((o - SPH_C) ** 2).sum() - SPH_R ** 2)
    with np.errstate(invalid="ignore"):
        t_true = (-b - np.sqrt(disc)) / a
        normal = (o + t_true[..., None] * dw - SPH_C) / SPH_R
        cosine = -(normal * dw).sum(-1) / np.sqrt(a)
    steep = (disc > 0) & (cosine >= 0.5)
    assert steep.sum() > 300
    for T, extra in ((np.float64, 0.0), (np.float32, PLANE_FP32_BOUND * 2)):      # t and g * voxel up to 5 m here
        out = RR.raycast(sphere_volume, SPH_VIEW[None], INTR, HW, SPH_LO, SPH_H, step=SPH_STEP, dtype=T)
        d = out["depth"][0].astype(np.float64)
        assert (d[steep] > 0).all() and not d[disc < -0.05].any()
        err = np.abs(d - t_true)[steep].max()
        n_err = np.abs(out["normal"][0].astype(np.float64) - normal)[steep].max()
        print(f"sphere {T.__name__}: {steep.sum()} rays, depth error {err:.3e} m (bound {bound + extra:.3e}), "
              f"normal error {n_err:.3e}")
        assert err <= bound + extra
        # a distance field's gradient has unit length; the interpolant's differs from it by at most h / rho per
        # component (the second derivatives times the cell), and the hit point by `bound` along the ray
        assert n_err <= h / rho + bound / rho + 1e-6
        assert (np.abs(np.linalg.norm(out["normal"][0][steep].astype(np.float64), axis=-1) - 1) <= 4 * EPS).all()


# ---- edge cases on a slab ---------------------------------------------------------------------------------------------
VOX = 0.125
S_DIMS, S_LO = (17, 13, 21), (-1.0, -0.75, 0.0)                # x in [-1, 1], y in [-0.75, 0.75], z in [0, 2.5]
S_INTR = (40.0, 40.0, 16.0, 12.0)                              # integer cx, cy: pixel (16, 12) looks along the axis
S_HW = (24, 32)


def slab(z_surface, seen_from=0, seen_to=None):
    """tsdf = clamp((z_surface - z) / trunc): free space in front (small z), weight 1 on z-indices [seen_from, seen_to)
    and tsdf = +1, weight 0 elsewhere, as fusion leaves never-observed points."""
    z = S_LO[2] + np.arange(S_DIMS[2]) * VOX
    prof = np.clip((z_surface - z) / (4 * VOX), -1.0, 1.0).astype(np.float32)
    seen = np.zeros(S_DIMS[2], bool)
    seen[seen_from:seen_to] = True
    g = np.random.default_rng(0)
    return {"tsdf": np.broadcast_to(np.where(seen, prof, 1.0).astype(np.float32), S_DIMS).copy(),
            "weight": np.broadcast_to(seen.astype(np.float32), S_DIMS).copy(),
            "colors": g.random((3,) + S_DIMS, dtype=np.float32)}


def cam(centre, R=np.eye(3)):
    return np.concatenate([np.asarray(R, np.float64), np.asarray(centre, np.float64)[:, None]], 1)[None]


def cast(vol, c2w, **kw):
    return RR.raycast(vol, c2w, S_INTR, S_HW, S_LO, VOX, **kw)


def assert_all_miss(out):
    assert not out["depth"].any() and not out["normal"].any() and not out["color"].any()


Z_S = 1.3125                                                   # between two lattice planes


def test_zero_direction_component_inside_the_slab_is_an_ordinary_ray():
    """Identity rotation, integer cx: column 16 has dx == 0 exactly, its x never changes.  With the centre's x inside
    [-1, 1] the axis constrains nothing: the column hits the plane at depth z_s - o.z like its neighbours."""
    out = cast(slab(Z_S), cam((0.1, 0.05, -0.5)))
    col = out["depth"][0][:, 16]
    assert (col > 0).all() and np.abs(col.astype(np.float64) - (Z_S + 0.5)).max() <= PLANE_FP32_BOUND
    assert np.array_equal(out["normal"][0][12, 16], np.array([0, 0, -1], np.float32))


def test_zero_direction_component_outside_the_slab_misses():
    """The same camera moved to x = -1.5: column 16 runs beside the box for ever (a miss, not a NaN from 0 * inf),
    columns to its right enter the box and hit."""
    out = cast(slab(Z_S), cam((-1.5, 0.05, -0.5)))
    assert not out["depth"][0][:, :17].any() and not out["normal"][0][:, :17].any()
    assert (out["depth"][0][:, 24:] > 0).any() and np.isfinite(out["depth"]).all()


def test_camera_looking_away_misses_everywhere():
    assert_all_miss(cast(slab(Z_S), cam((0.1, 0.05, -0.5), np.diag([-1.0, 1.0, -1.0]))))


def test_camera_inside_never_observed_space_sees_the_observed_surface():
    """z-indices below 6 (z < 0.75) were never observed; the camera sits among them at z = 0.3.  Its samples there are
    invalid and cannot be an end of a hit; the surface at 1.3125 lies in observed space and is found at depth 1.0125."""
    out = cast(slab(Z_S, seen_from=6), cam((0.0, 0.0, 0.3)))
    d = out["depth"][0]
    assert (d[8:16, 12:20] > 0).all()
    assert np.abs(d[d > 0].astype(np.float64) - (Z_S - 0.3)).max() <= PLANE_FP32_BOUND


def test_min_weight_above_every_weight_misses_everywhere():
    assert_all_miss(cast(slab(Z_S), cam((0.1, 0.05, -0.5)), min_weight=2.0))


def test_a_sample_exactly_on_the_zero_level_starts_the_hit():
    """Surface on the lattice plane z = 1.25, camera at z = -0.25 on the axis of pixel (16, 12), step 0.5: t_i = 0.25 +
    i / 16 and g.z = i / 2 are exact, so f_20 == 0 exactly.  f_20 is not < 0, so i = 20 is no hit; at i = 21 f_20 >= 0
    and f_21 < 0: t* = t_20 + dt * (0 / (0 - f_21)) = 1.5 exactly, normal exactly (0, 0, -1)."""
    vol = slab(1.25)
    assert (vol["tsdf"][:, :, 10] == 0).all()
    out = cast(vol, cam((0.0, 0.0, -0.25)))
    assert out["depth"][0][12, 16] == np.float32(1.5)
    assert np.array_equal(out["normal"][0][12, 16], np.array([0, 0, -1], np.float32))


def test_back_face_only_ray_misses():
    """From inside the solid (z = 2.2, tsdf < 0) looking back along -z every ray goes from negative to positive: never a
    hit.  The same with the solid never observed (weight 0, tsdf +1 behind the band), as fusion leaves it."""
    back = np.diag([-1.0, 1.0, -1.0])
    assert_all_miss(cast(slab(Z_S), cam((0.0, 0.0, 2.2), back)))
    assert_all_miss(cast(slab(Z_S, seen_to=15), cam((0.0, 0.0, 2.2), back)))


def test_near_and_far_clip_the_march():
    """The surface is at depth 1.8125 for every pixel.  near = 2 starts behind it (first sample already negative: no
    front crossing), far = 1.5 ends before it; [1, 2] contains it and gives the unclipped hits."""
    vol, c2w = slab(Z_S), cam((0.1, 0.05, -0.5))
    full = cast(vol, c2w)
    assert_all_miss(cast(vol, c2w, near=2.0))
    assert_all_miss(cast(vol, c2w, far=1.5))
    clipped = cast(vol, c2w, near=1.0, far=2.0)
    assert np.array_equal(clipped["depth"] > 0, full["depth"] > 0) and (full["depth"] > 0).any()
    assert np.abs(clipped["depth"].astype(np.float64) - full["depth"]).max() <= PLANE_FP32_BOUND


def test_nan_pose_gives_an_all_zero_frame_and_leaves_its_neighbour_alone():
    good = cam((0.1, 0.05, -0.5))
    for r, c in ((0, 0), (1, 3), (2, 2)):
        bad = good.copy()
        bad[0, r, c] = np.nan
        out = cast(slab(Z_S), np.concatenate([bad, good]))
        assert not out["depth"][0].any() and not out["normal"][0].any() and not out["color"][0].any()
        assert (out["depth"][1] > 0).any()
    inf = good.copy()
    inf[0, 2, 3] = np.inf
    assert_all_miss(cast(slab(Z_S), inf))


# ---- brick skipping --------------------------------------------------------------------------------------------------
def test_brick_flags_rule():
    """One negative point at (8, 8, 16) of a 37 x 21 x 70 lattice: it is a corner of the cells of bricks 0 and 1 along
    x and y and of bricks 1 and 2 along z, and of no others.  70 points make ceil(69 / 8) = 9 bricks, the last partial."""
    tsdf = np.ones((37, 21, 70), np.float32)
    tsdf[8, 8, 16] = -0.5
    flags = RR.brick_flags(tsdf)
    assert flags.shape == (5, 3, 9) == RR.brick_dims(tsdf.shape)
    want = np.zeros_like(flags)
    want[0:2, 0:2, 1:3] = 1
    assert np.array_equal(flags, want)
    tsdf[:] = 1.0
    tsdf[36, 20, 69] = -0.0                                    # -0 is not < 0
    assert not RR.brick_flags(tsdf).any()
    tsdf[36, 20, 69] = -1e-30
    assert RR.brick_flags(tsdf).sum() == 1 and RR.brick_flags(tsdf)[4, 2, 8] == 1


def same_bits(a, b):
    return all((a[k] is None and b[k] is None) or np.array_equal(a[k].view(np.int32), b[k].view(np.int32)) for k in a)


def test_skipped_march_equals_the_plain_march(plane_case, sphere_volume):
    cases = [(plane_case[np.float32][0], PLANE_VIEW[None], INTR, HW, TR.PLANE_BOUND[:, 0], TR.PLANE_VOXEL),
             (sphere_volume, SPH_VIEW[None], INTR, HW, SPH_LO, SPH_H),
             (slab(Z_S, seen_from=6), np.concatenate([cam((0.0, 0.0, 0.3)), cam((-1.5, 0.05, -0.5)),
                                                      cam((0.0, 0.0, 2.2), np.diag([-1.0, 1.0, -1.0]))]),
              S_INTR, S_HW, S_LO, VOX)]
    for vol, c2w, intr, size, lo, voxel in cases:
        flags = RR.brick_flags(np.asarray(vol["tsdf"]).astype(np.float32))
        assert 0 < flags.sum() < flags.size                    # the skip is exercised
        for step in (1.0, 0.5, 0.3):
            plain, skipped, stats = {}, {}, {}
            a = RR.raycast(vol, c2w, intr, size, lo, voxel, step=step, stats=plain)
            b = RR.raycast(vol, c2w, intr, size, lo, voxel, step=step, flags=flags, stats=skipped)
            assert same_bits(a, b)
            assert plain["evaluated"] == plain["samples"] == skipped["samples"]
            assert skipped["evaluated"] < plain["evaluated"]


def test_lerp_chain_of_non_negative_corners_is_never_negative():
    """The skip's premise, tried where rounding is most likely to break it: corners a few ulps apart and fractions next
    to 0 and 1."""
    g = np.random.default_rng(11)
    base = g.random(4000).astype(np.float32) * np.float32(1e-3)
    for scale in (1e-38, 1e-7, 1.0):
        v = [[[np.abs(base + g.integers(-3, 4, base.shape) * np.spacing(base)).astype(np.float32) * np.float32(scale)
               for _ in (0, 1)] for _ in (0, 1)] for _ in (0, 1)]
        for s in (g.random(base.shape).astype(np.float32), np.float32(1) - np.float32(2.0 ** -24) * np.ones_like(base),
                  np.full_like(base, 2.0 ** -30)):
            f = RR._trilinear(v, [s, s[::-1].copy(), s])
            assert not (f < 0).any()


# ---- the Python surface ----------------------------------------------------------------------------------------------
def test_c2w_matrices_is_the_float64_inverse_rounded_once():
    from go_slam_amd.lietorch_shim import SE3
    from go_slam_amd.tsdf import c2w_matrices, w2c_matrices
    from go_slam_amd import synth
    poses = synth.arc_poses(9)                                 # [9,7] float32
    m44 = SE3(poses.double()).matrix()
    want = np.linalg.inv(m44.numpy())[:, :3, :]
    for form in (poses, m44, m44[:, :3, :]):
        got = c2w_matrices(form)
        assert got.dtype == torch.float32 and tuple(got.shape) == (9, 3, 4) and got.is_contiguous()
        assert (np.abs(got.numpy().astype(np.float64) - want) <= EPS * np.abs(want) + 1e-12).all()
    assert np.array_equal(w2c_matrices(m44).numpy(), m44[:, :3, :].float().numpy())
    with pytest.raises(ValueError):
        c2w_matrices(torch.zeros(3, 6))


def test_raycast_refuses_bad_arguments_before_touching_the_device(built_lib):
    from go_slam_amd.tsdf import TSDFVolume
    vol = TSDFVolume([[0, 1], [0, 1], [0, 1]], 0.25, device="cpu")
    pose = torch.eye(4)[None]
    intr = (40.0, 40.0, 16.0, 12.0)
    for kw in ({"size": (0, 4)}, {"size": (4,)}, {"near": -1.0}, {"near": 2.0, "far": 2.0}, {"step": 0.0},
               {"step": 1.5}, {"step": 1e-9}, {"near": float("nan")}):
        args = {"size": (4, 4), **kw}
        with pytest.raises(ValueError):
            vol.raycast(pose, intr, **args)
    with pytest.raises(ValueError):
        vol.raycast(pose, (40.0, 40.0, 16.0), (4, 4))
    with pytest.raises(ValueError):
        vol.raycast(pose, (0.0, 40.0, 16.0, 12.0), (4, 4))
    with pytest.raises(ValueError):
        vol.raycast(torch.zeros(2, 5), intr, (4, 4))


def test_library_refuses_bad_arguments_and_launches_nothing(built_lib):
    """Every check of the header comes before any launch, so null pointers are never reached."""
    from go_slam_amd import _lib
    L = _lib.lib()
    inf = float("inf")

    def call(dims=(9, 9, 9), k=1, h=4, w=4, fx=40.0, voxel=0.1, near=0.0, far=inf, step=0.5):
        return L.gs_tsdf_raycast(None, None, None, *dims, None, None, k, h, w, fx, 40.0, 2.0, 2.0, 0.0, 0.0, 0.0, voxel,
                                 near, far, step, 1.0, None, None, None, None)

    for kw in ({"dims": (1, 9, 9)}, {"dims": (9, 1025, 9)}, {"h": 0}, {"w": 0}, {"k": -1}, {"step": 0.0},
               {"step": 1.0000001}, {"step": float("nan")}, {"step": 1e-7}, {"voxel": 0.0}, {"voxel": -1.0},
               {"near": -0.5}, {"near": 1.0, "far": 1.0}, {"far": float("nan")}, {"fx": 0.0}):
        assert call(**kw) == -1, kw
        assert L.gs_last_error().startswith(b"tsdf_raycast")
    assert call(k=0) == 0                                      # K == 0: nothing to do, not an error
    assert call() == -1 and b"null pointer" in L.gs_last_error()
    assert L.gs_tsdf_brick_flags_bytes(37, 21, 70) == 5 * 3 * 9
    assert L.gs_tsdf_brick_flags_bytes(2, 2, 2) == 1 and L.gs_tsdf_brick_flags_bytes(1024, 1024, 9) == 128 * 128
    assert L.gs_tsdf_brick_flags_bytes(1, 8, 8) == 0
    assert L.gs_tsdf_brick_flags(None, 0, 9, 9, None, None) == -1


def test_metrics_tsdf_depth_text_round_trip():
    from go_slam_amd import tsdf
    frames = [0, 5, 10]
    per_frame = np.array([[0.0123456789012345, 2999 / 3072, 2999, 3072], [float("nan"), 0.0, 0, 2000],
                          [1 / 3, 1.0, 17, 17]])
    res = tsdf.summarize_depth(frames, per_frame)
    assert res["n_frames"] == 3
    assert res["depth_l1_cm"] == 100.0 * ((0.0123456789012345 + 1 / 3) / 2)        # the frame without a pair is left out
    assert res["coverage"] == ((2999 / 3072 + 0.0) + 1.0) / 3
    text = tsdf.depth_metrics_text(res, frames, per_frame)
    back, rows = tsdf.parse_depth_metrics(text)
    assert back == res
    assert [r[0] for r in rows] == frames and [r[3] for r in rows] == [2999, 0, 17]
    assert rows[0][1] == per_frame[0, 0] and rows[2][1] == per_frame[2, 0] and math.isnan(rows[1][1])
    assert [r[2] for r in rows] == list(per_frame[:, 1])
    empty = tsdf.summarize_depth([], np.zeros((0, 4)))
    text = tsdf.depth_metrics_text(empty, [], np.zeros((0, 4)), metric_depth=False)
    assert "not rgbd" in text.splitlines()[1]
    back, rows = tsdf.parse_depth_metrics(text)
    assert rows == [] and back["n_frames"] == 0 and math.isnan(back["depth_l1_cm"]) and math.isnan(back["coverage"])
    with pytest.raises(ValueError):
        tsdf.parse_depth_metrics("something else\n")
