"""Plane finding without a GPU (go_slam_amd/tsdf_planes.py over tests/tsdf_planes_restatement.py): the surface sample of a
cell lies on an analytic plane to fp32 rounding, the cube map's ties and the sample rule's skips behave as
include/goslam_hip.h writes them, the floor policy and the upright transform do what they state, the text round trip is
exact, bad arguments are refused before the library is reached, and the restated pipeline recovers the wall and the
floor of tests/test_tsdf_gpu.py's scene fused in a world tilted by 20 degrees of roll and 10 of pitch, stands the volume
upright on the floor, and only then is a slab above the floor free of it."""
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from go_slam_amd import synth                                  # noqa: E402
from go_slam_amd import tsdf_planes as TP                      # noqa: E402
import esdf_restatement as ER                                  # noqa: E402
import tsdf_align_restatement as AR                            # noqa: E402
import tsdf_merge_restatement as MR                            # noqa: E402
import tsdf_planes_restatement as PR                           # noqa: E402
import tsdf_restatement as TR                                  # noqa: E402

F = np.float32
EPS = float(np.finfo(np.float32).eps)
VOXEL = 0.125                                                  # tests/test_tsdf_gpu.py's lattice: 37 x 21 x 70
BOUND = [[-1.5, 3.0], [-0.75, 1.75], [-2.0, 6.625]]
DIMS, LO, TRUNC = (37, 21, 70), [b[0] for b in BOUND], 4 * VOXEL
H, W = 48, 64
INTR = (0.9 * W, 0.9 * W, W / 2 - 0.5, H / 2 - 0.5)
CHUNK = 2048                                                   # gs_tsdf_align_chunk; the GPU suite reads it from the library
SLAB = (0.2, 1.0)                                              # metres above the floor


# ---- the scene in a tilted world ----------------------------------------------------------------------------------------
def four(m):
    out = np.eye(4)
    out[:3, :] = np.asarray(m, np.float64)[:3, :]
    return out


def tilt():
    """float64 [4,4], the scene's own world D to the tilted world S: 10 degrees of pitch (about x), then 20 of roll (about
    z), about the middle of the lattice's box so that the scene stays inside it."""
    R = AR.rotation([0.0, 0.0, math.radians(20.0)]) @ AR.rotation([math.radians(10.0), 0.0, 0.0])
    c = np.array([0.5 * (b[0] + b[1]) for b in BOUND])
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = R, c - R @ c
    return M


def truth(M):
    """The wall z = 4 and the floor y = 1.2 of synth's scene in the world x_S = M x_D, normals toward free space:
    {"wall": (n, o), "floor": (n, o)} with n . x = o."""
    out = {}
    for name, n, o in (("wall", np.array([0.0, 0.0, -1.0]), -4.0), ("floor", np.array([0.0, -1.0, 0.0]), -1.2)):
        ns = M[:3, :3] @ n
        out[name] = (ns, o + float(ns @ M[:3, 3]))
    return out


def arc_inputs(K, M):
    """tests/test_tsdf_gpu.py's arc frames (depth, w2c float32 [K,3,4], mask) for the world x_S = M x_D: a camera that
    sees x_D = M^-1 x_S has the world-to-camera matrix W M^-1, formed in float64 and rounded once."""
    from go_slam_amd.tsdf import w2c_matrices
    poses = synth.arc_poses(K)
    disp = synth.plane_disps(poses, torch.tensor(INTR), H, W)
    depth = torch.where(disp > 0, 1.0 / disp, torch.zeros_like(disp))
    g = torch.Generator().manual_seed(7)
    depth[torch.rand(K, H, W, generator=g) < 0.05] = 0.0
    mask = (torch.rand(K, H, W, generator=g) > 0.2).float()
    Minv = np.linalg.inv(M)
    w2c = np.stack([(four(m) @ Minv)[:3, :] for m in w2c_matrices(poses).numpy()]).astype(np.float32)
    return depth.numpy(), w2c, mask.numpy()


def restated_volume(K, M):
    depth, w2c, mask = arc_inputs(K, M)
    vol = TR.integrate(TR.new_volume(DIMS), depth, w2c, INTR, LO, VOXEL, TRUNC, 64.0, images=None, mask=mask)
    return MR.volume(vol["tsdf"], vol["weight"], LO, VOXEL, TRUNC)


def plane_points(vol, n, o, cone_deg=10.0, band=VOXEL):
    """float64 [N,3]: the restated surface samples within `band` of the plane n . x = o whose direction agrees with n."""
    s = PR.samples(vol)
    nf = np.asarray(n, np.float64).astype(F)
    ok = PR.agrees(s, nf, math.cos(math.radians(cone_deg)) ** 2) & (np.abs(PR.along(s, nf) - F(o)) <= F(band))
    return s["p"][ok].astype(np.float64)


def shorter_side(points, n):
    """The shorter observed side of a plane: the smaller extent of its points along the two principal axes of their spread
    inside the plane."""
    c = points - points.mean(0)
    c = c - np.outer(c @ n, n)
    axes = np.linalg.eigh(c.T @ c)[1][:, 1:]                    # the two in-plane directions (the smallest is n)
    return min(float(np.ptp(c @ axes[:, k])) for k in range(2))


def slab_cells(vol, axis, h0, h1):
    """ESDF.occupancy_slice's cells of the lattice layers with h0 <= lo + k voxel <= h1 along `axis`, robot radius 0,
    known_fraction 0.5 (tests/esdf_restatement.py)."""
    e = ER.build(vol["tsdf"], vol["weight"], 1023, vol["voxel"])
    top = vol["tsdf"].shape[axis] - 1
    k0 = int(max(math.ceil((h0 - vol["lo"][axis]) / vol["voxel"]), 0))
    k1 = int(min(math.floor((h1 - vol["lo"][axis]) / vol["voxel"]), top))
    return ER.occupancy_slice(e["state"], e["d2"], e["dist"], axis, k0, k1, 0, int(math.ceil(0.5 * (k1 - k0 + 1))))[0]


def footprint(lo, dims, voxel, points, axis):
    """bool [n_u,n_v]: the columns along `axis` (the two other axes in increasing order) that hold one of `points`."""
    u, v = [a for a in range(3) if a != axis]
    iu = np.rint((points[:, u] - lo[u]) / voxel).astype(int)
    iv = np.rint((points[:, v] - lo[v]) / voxel).astype(int)
    out = np.zeros((dims[u], dims[v]), bool)
    out[iu, iv] = True
    return out


def floor_area_points(vol, floor, wall):
    """The floor's sample points that stand clear of the wall: more than 1.5 voxels in front of it.  (A wall stands on its
    floor: the columns under it are the wall's.  Its sites reach one voxel in front of the surface, and a point is half a
    voxel from its column's middle at most.)"""
    pts = plane_points(vol, floor["normal"], floor["offset"])
    return pts[pts @ wall["normal"] - wall["offset"] > 1.5 * vol["voxel"]]


def tilted_slab_share(vol, floor, wall, axis):
    """The share of the floor's columns along lattice axis `axis` of the tilted volume that the slab SLAB above the
    floor's centroid (along that axis, on the floor's free side) shows occupied."""
    sign = 1.0 if floor["normal"][axis] > 0 else -1.0
    h = sorted(floor["centroid"][axis] + sign * s for s in SLAB)
    cells = slab_cells(vol, axis, *h)
    fp = footprint(vol["lo"], vol["tsdf"].shape, vol["voxel"], floor_area_points(vol, floor, wall), axis)
    return float((cells[fp] == 0).mean()), int(fp.sum())


def assert_upright_map(cells, fp):
    """The upright map's slab: no column of the floor's footprint occupied, and the wall one straight band along the
    map's first axis: at most trunc / voxel + 2 columns wide, every row of it one run."""
    assert fp.sum() > 100 and (cells[fp] == 0).sum() == 0 and (cells[fp] == 254).mean() > 0.9
    occ = np.argwhere(cells == 0)
    rows = np.unique(occ[:, 0])
    assert len(rows) > 20 and np.array_equal(rows, np.arange(rows[0], rows[-1] + 1))
    assert occ[:, 1].max() - occ[:, 1].min() + 1 <= TRUNC / VOXEL + 2
    for r in rows:
        cols = occ[occ[:, 0] == r, 1]
        assert np.array_equal(cols, np.arange(cols[0], cols[-1] + 1))


@pytest.fixture(scope="module")
def tilted():
    M = tilt()
    vol = restated_volume(33, M)
    planes = PR.find_planes(vol, CHUNK)
    return {"M": M, "vol": vol, "planes": planes, "truth": truth(M), "up": M[:3, :3] @ np.array([0.0, -1.0, 0.0])}


# ---- the surface sample ---------------------------------------------------------------------------------------------------
def analytic_volume(n, o, dims=DIMS, lo=LO, voxel=VOXEL, trunc=TRUNC):
    ax = [lo[a] + voxel * np.arange(dims[a], dtype=np.float64) for a in range(3)]
    P = np.stack(np.meshgrid(*ax, indexing="ij"), -1)
    return MR.volume(np.clip((P @ n - o) / trunc, -1.0, 1.0), np.ones(dims), lo, voxel, trunc)


@pytest.mark.parametrize("rotvec, o", [((0.3, -0.2, 0.1), 1.9), ((-0.5, 0.4, 0.25), 2.4), ((1.1, 0.7, -0.4), 0.6)])
def test_samples_of_an_analytic_plane_lie_on_it(rotvec, o):
    """f = (n . x - o) / trunc is linear: the trilinear value and gradient and the Newton step are exact up to rounding, so
    every sample lies within 4 eps |x|max of the plane and its direction is n."""
    n = AR.rotation(rotvec) @ np.array([0.0, 0.0, 1.0])
    s = PR.samples(analytic_volume(n, o))
    p, g = s["p"][s["is"]].astype(np.float64), s["g"][s["is"]].astype(np.float64)
    xmax = max(abs(v) for b in BOUND for v in b)
    err = np.abs(p @ n - o).max()
    print(f"{len(p)} samples, largest distance {err:.3e} m against {4 * EPS * xmax:.3e}")
    assert len(p) > 500 and err <= 4 * EPS * xmax
    assert np.abs(g / np.linalg.norm(g, axis=1, keepdims=True) - n).max() < 1e-5
    assert np.abs(np.linalg.norm(g, axis=1) - VOXEL / TRUNC).max() < 1e-5      # in lattice units: voxel / trunc per voxel


@pytest.mark.parametrize("axis, sign", [(0, 1), (1, -1), (2, 1), (2, -1)])
def test_an_axis_aligned_plane_votes_into_one_face(axis, sign):
    n = np.zeros(3)
    n[axis] = float(sign)
    vol = analytic_volume(n, sign * 0.51)
    v = PR.votes(vol, 16)
    face = 2 * axis + (sign < 0)
    assert v.sum() == PR.samples(vol)["is"].sum() > 500 and v[face].sum() == v.sum()
    assert v[face, 8, 8] == v.sum()                             # u = v = 0 exactly: bin floor(1 * 8)


def one_cell(values, weights=None):
    """The 2 x 2 x 2 lattice with the corner values [i][j][k]."""
    return MR.volume(np.asarray(values, np.float64).reshape(2, 2, 2),
                     np.ones((2, 2, 2)) if weights is None else np.asarray(weights, np.float64).reshape(2, 2, 2),
                     (0.0, 0.0, 0.0), 1.0, 4.0)


def test_cube_map_ties_and_the_sample_rules_skips():
    i, j, k = np.meshgrid([0, 1], [0, 1], [0, 1], indexing="ij")
    tie = one_cell(0.25 * (i + j - 1))                          # g = (0.25, 0.25, 0): the lowest axis wins
    s = PR.samples(tie)
    assert s["is"].all() and s["g"][0].tolist() == [0.25, 0.25, 0.0] and s["f"][0] == 0 and s["p"][0].tolist() == [0.5, 0.5, 0.5]
    assert np.argwhere(PR.votes(tie, 16)).tolist() == [[0, 15, 8]]        # u = +1 lands in the last bin, not past it
    assert np.argwhere(PR.votes(one_cell(-0.25 * (i + j - 1)), 16)).tolist() == [[1, 0, 8]]
    assert np.argwhere(PR.votes(one_cell(0.25 * (j + k - 1)), 2)).tolist() == [[2, 1, 1]]   # |g1| = |g2|: axis 1, (g0, g2)
    assert np.argwhere(PR.votes(one_cell(0.25 * (i - k)), 4)).tolist() == [[0, 2, 0]]       # |g0| = |g2|: axis 0, v = -1
    step = one_cell(0.25 * (i + j - 1) + 0.125)                 # f = 0.125: half a voxel along (1, 1, 0) / sqrt 2
    s = PR.samples(step)
    assert s["is"].all() and s["p"][0].tolist() == [0.25, 0.25, 0.5]
    far = np.full((2, 2, 2), 0.5)
    far[0, 0, 0] = -0.01                                        # a sign change, but the zero set is a corner's nick
    s = PR.samples(one_cell(far))
    assert not s["is"].any() and s["f"][0] ** 2 > s["gg"][0] > 0
    saddle = one_cell(0.5 * (-1.0) ** (i + j + k))              # a sign change without a gradient at the centre
    s = PR.samples(saddle)
    assert not s["is"].any() and s["gg"][0] == 0 and s["f"][0] == 0
    good = 0.25 * (i + j - 1)
    for bad in (math.nan, 1.0, -1.0):
        v = good.astype(np.float64).copy()
        v[1, 0, 1] = bad
        assert not PR.samples(one_cell(v))["is"].any(), bad
    w = np.ones((2, 2, 2))
    w[0, 1, 0] = 0.0
    assert not PR.samples(one_cell(good, w))["is"].any()
    w[0, 1, 0] = math.nan
    assert not PR.samples(one_cell(good, w))["is"].any()
    assert PR.samples(one_cell(good, 2 * np.ones(8)), min_weight=2.0)["is"].all()
    assert not PR.samples(one_cell(good, 2 * np.ones(8)), min_weight=2.5)["is"].any()
    assert not PR.samples(one_cell(np.full(8, 0.25)))["is"].any() and not PR.samples(one_cell(np.full(8, -0.25)))["is"].any()
    assert not PR.votes(saddle, 16).any() and not PR.offsets(saddle, [[0, 0, 1.0]], [0.0], 0.9, 0.5, 8).any()


def test_offsets_and_moments_of_an_analytic_plane():
    """Along its own normal every sample of a plane falls into the bin that holds o; a direction outside the cone gets
    none; the moments' centroid lies on the plane and the residual sum is rounding."""
    n = AR.rotation((0.3, -0.2, 0.1)) @ np.array([0.0, 0.0, 1.0])
    vol = analytic_volume(n, 1.9)
    count = int(PR.samples(vol)["is"].sum())
    cos2 = math.cos(math.radians(10.0)) ** 2
    away = AR.rotation((0.0, math.radians(25.0), 0.0)) @ n
    hist = PR.offsets(vol, [n, away, -n], [1.9 - 10.5 * VOXEL] * 3, cos2, VOXEL, 32)
    assert hist[0, 10] == count and hist.sum() == count
    assert PR.offsets(vol, [n], [1.9 - 0.25 * VOXEL], cos2, VOXEL, 1).sum() == count
    assert PR.offsets(vol, [n], [1.9 + 0.5 * VOXEL], cos2, VOXEL, 4).sum() == 0           # kf = -1 is dropped
    ref = TP.box_centre32(DIMS, LO, VOXEL)
    rows = PR.moments(vol, [[*n, 1.9], [*away, 1.9], [*n, 2.9]], cos2, VOXEL, ref, CHUNK)
    assert rows[0, 10] == rows[0, 11] == rows[2, 11] == count and rows[1, 10] == rows[1, 11] == rows[2, 10] == 0
    assert not rows[1, :10].any() and not rows[:, 12:].any()
    centroid = ref.astype(np.float64) + rows[0, :3] / count
    assert abs(centroid @ n - 1.9) < 1e-6 and math.sqrt(rows[0, 9] / count) < 1e-6
    fit = TP.planes_update(rows[:1], np.array([[*away, 0.0]]), n[None], ref.astype(np.float64))
    assert math.degrees(math.acos(min(1.0, fit[0, :3] @ n))) < 1e-4 and abs(fit[0, 3] - 1.9) < 1e-6
    assert PR.moments(vol, [[*n, 1.9]], cos2, VOXEL, ref, CHUNK).view(np.int64).tolist() == rows[:1].view(np.int64).tolist()


# ---- the host steps -----------------------------------------------------------------------------------------------------
def test_vote_peaks_finds_separate_directions_in_order():
    C = TP.cube_centres(16)
    votes = np.zeros(6 * 16 * 16, np.uint32)
    a, b = AR.rotation((0.2, 0.1, 0.0)) @ np.array([0, 0, 1.0]), AR.rotation((0.0, -0.3, 0.1)) @ np.array([0, -1.0, 0])
    for d, cnt in ((a, 50), (b, 300)):
        near = np.argsort(-(C @ d))[:4]
        votes[near] += np.array([4, 3, 2, 1], np.uint32) * cnt
    votes[5] = 9                                                # a few stray votes: below min_cells
    peaks = TP.vote_peaks(votes.reshape(6, 16, 16), 10.0, 8, 64)
    assert peaks.shape == (2, 3)
    assert math.degrees(math.acos(peaks[0] @ b)) < 3.0 and math.degrees(math.acos(peaks[1] @ a)) < 3.0
    assert TP.vote_peaks(votes.reshape(6, 16, 16), 10.0, 1, 64).shape == (1, 3)
    assert TP.vote_peaks(np.zeros((6, 4, 4), np.uint32), 10.0, 8, 1).shape == (0, 3)


def test_offset_hypotheses_are_the_local_maxima_of_the_three_bin_sum():
    h = np.zeros((2, 12), np.uint32)
    h[0, 2:4] = (50, 60)                                        # one plane across two bins
    h[0, 8] = 70
    h[1, 5] = 200
    h[1, 10] = 5                                                # below min_cells
    n = np.array([[0, 0, 1.0], [0, 1.0, 0]])
    planes, source = TP.offset_hypotheses(h, n, np.array([-1.0, 2.0]), 0.5, 10, 8)
    assert source.tolist() == [1, 0, 0] and planes[:, :3].tolist() == [[0, 1, 0], [0, 0, 1], [0, 0, 1]]
    assert planes[0, 3] == 2.0 + 0.5 * 5.5 and planes[2, 3] == -1.0 + 0.5 * 8.5
    assert planes[1, 3] == -1.0 + 0.5 * (50 * 2.5 + 60 * 3.5) / 110
    assert TP.offset_hypotheses(h, n, np.array([-1.0, 2.0]), 0.5, 10, 2)[1].tolist() == [1, 0]


def plane(n, o, count, centroid=None):
    n = np.asarray(n, np.float64) / np.linalg.norm(n)
    return {"normal": n, "offset": float(o), "count": count, "rmse_m": 0.01, "area_m2": 1.0,
            "centroid": o * n if centroid is None else np.asarray(centroid, np.float64)}


def test_floor_plane_is_the_lowest_large_level_plane():
    up = [0.0, -1.0, 0.0]                                       # y grows downward, as in a camera's frame
    floor, table, wall = plane([0, -1, 0], -1.2, 400), plane([0.05, -1, 0], -0.4, 900), plane([0, 0, -1], -4.0, 5000)
    ceiling, crumb, ramp = plane([0, 1, 0], -1.5, 800), plane([0, -1, 0], -1.6, 100), plane([0.8, -1, 0], -3.0, 2000)
    assert TP.floor_plane([wall, table, floor, ceiling], up) is floor
    assert TP.floor_plane([wall, table, floor, crumb], up) is floor            # 100 < a quarter of 900: not a floor
    assert TP.floor_plane([wall, table, floor, crumb], up, min_share=0.1) is crumb
    assert TP.floor_plane([wall, ramp, table], up) is table                    # 38.7 degrees off: too steep
    assert TP.floor_plane([wall, ramp, table], up, max_tilt_deg=45) is ramp
    assert TP.floor_plane([wall, ceiling], up) is None and TP.floor_plane([], up) is None
    assert TP.floor_plane([wall, ceiling], [0, 2.0, 0]) is ceiling             # a world whose up is +y
    for bad in (dict(up_hint=[0, 0, 0]), dict(up_hint=[1, 2]), dict(up_hint=[math.nan, 0, 1]), dict(max_tilt_deg=90),
                dict(min_share=1.5), dict(min_share=-0.1)):
        with pytest.raises(ValueError, match="floor_plane"):
            TP.floor_plane([floor], **dict(dict(up_hint=up), **bad))
    with pytest.raises(ValueError, match="plane 0"):
        TP.floor_plane([{"normal": [0, 2.0, 0], "offset": 1.0}], up)


@pytest.mark.parametrize("up_axis", [0, 1, 2])
@pytest.mark.parametrize("up_sign", [1, -1])
def test_upright_transform_puts_the_plane_at_zero(up_axis, up_sign):
    from go_slam_amd.tsdf_merge import transforms34
    rng = np.random.default_rng(5)
    e = np.zeros(3)
    e[up_axis] = up_sign
    normals = [rng.normal(size=3) for _ in range(4)] + [e, -e, -e + [1e-9, 0, 0], [0.6, 0, 0.8]]
    for n in normals:
        n = np.asarray(n, np.float64) / np.linalg.norm(n)
        o = float(rng.uniform(-3, 3))
        T = TP.upright_transform({"normal": n, "offset": o}, up_axis, up_sign)
        transforms34(T, "test")                                 # rigid
        assert np.abs(T[:3, :3] @ n - e).max() < 1e-12
        t1, t2 = np.linalg.svd(n[None])[2][1:]
        x = o * n + rng.normal(size=(50, 1)) * t1 + rng.normal(size=(50, 1)) * t2
        y = x @ T[:3, :3].T + T[:3, 3]
        assert np.abs(y[:, up_axis]).max() < 1e-12
        assert ((x + 0.3 * n) @ T[:3, :3].T + T[:3, 3])[:, up_axis] == pytest.approx(0.3 * up_sign, abs=1e-12)
        if abs(n @ e) < 1 - 1e-6:                               # the smallest rotation: about n x e, by their angle
            ang = math.degrees(math.acos((np.trace(T[:3, :3]) - 1) / 2))
            assert ang == pytest.approx(math.degrees(math.acos(n @ e)), abs=1e-6)
    assert np.array_equal(TP.upright_transform({"normal": e, "offset": 0.0}, up_axis, up_sign), np.eye(4))


def test_upright_transform_with_a_wall_faces_a_lattice_axis():
    floor = plane(AR.rotation((0.2, 0.1, -0.3)) @ np.array([0, -1.0, 0]), -1.2, 100)
    for deg in (-100.0, -44.0, 3.0, 44.0, 46.0, 170.0):
        t = AR.rotation(math.radians(deg) * floor["normal"]) @ np.linalg.svd(floor["normal"][None])[2][1]
        wall = plane(t + 0.05 * floor["normal"], 2.0, 50)       # a little off perpendicular
        T0, T = TP.upright_transform(floor, 2, 1), TP.upright_transform(floor, 2, 1, wall)
        h = T[:3, :3] @ wall["normal"]
        assert min(abs(h[0]), abs(h[1])) < 1e-12 and abs(h[2]) < 0.06
        assert np.abs(T[:3, :3] @ floor["normal"] - [0, 0, 1]).max() < 1e-12 and T[2, 3] == pytest.approx(T0[2, 3], abs=1e-12)
        turn = T[:3, :3] @ T0[:3, :3].T                         # about up, by 45 degrees at most
        assert np.abs(turn[2] - [0, 0, 1]).max() < 1e-12 and math.degrees(math.acos(min(1.0, turn[0, 0]))) <= 45 + 1e-9
    with pytest.raises(ValueError, match="not roughly perpendicular"):
        TP.upright_transform(floor, 2, 1, plane(floor["normal"] + [0.1, 0, 0], 0.0, 5))
    for bad in (dict(up_axis=3), dict(up_sign=0), dict(plane={"normal": [0, 0, 2.0], "offset": 0.0}),
                dict(plane={"normal": [0, 0, 1.0], "offset": math.nan}), dict(plane={"offset": 1.0})):
        with pytest.raises(ValueError, match="upright_transform"):
            TP.upright_transform(**dict(dict(plane=floor, up_axis=2, up_sign=1), **bad))


def test_text_round_trip_is_exact(tilted):
    planes = tilted["planes"]
    for floor in (None, planes[1]):
        text = TP.planes_text(planes, floor)
        back, index = TP.parse_planes(text)
        assert TP.planes_text(back, None if index is None else back[index]) == text
        assert index == (None if floor is None else 1) and len(back) == len(planes)
        for p, q in zip(planes, back):
            assert p["count"] == q["count"]
            for key in ("normal", "offset", "rmse_m", "centroid", "area_m2"):
                a, b = (np.ascontiguousarray(x[key], np.float64).view(np.int64) for x in (p, q))
                assert np.array_equal(a, b), key
    assert TP.parse_planes(TP.planes_text([])) == ([], None)
    for bad in ("", "something else\n", TP.planes_text(planes) + "1 2 3\n"):
        with pytest.raises(ValueError, match="metrics_tsdf_planes"):
            TP.parse_planes(bad)


def test_bad_arguments_are_refused_before_the_library(monkeypatch):
    from go_slam_amd import _lib
    from go_slam_amd.tsdf import TSDFVolume

    def unloaded():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "lib", unloaded)
    vol = TSDFVolume.__new__(TSDFVolume)
    vol.voxel, vol.lo, vol.dims, vol.trunc, vol.max_weight, vol.device = VOXEL, np.array(LO), DIMS, TRUNC, 64.0, "cuda:0"
    vol.tsdf = vol.weight = vol.colors = None
    for bad in (dict(bins=15), dict(bins=0), dict(bins=66), dict(bins=8.5), dict(cone_deg=0), dict(cone_deg=90),
                dict(cone_deg=math.nan), dict(band=0.0), dict(band=-1.0), dict(band=math.inf), dict(max_planes=0),
                dict(max_planes=17), dict(min_cells=0), dict(min_weight=math.nan), dict(min_weight=math.inf),
                dict(iterations=-1), dict(iterations=1.5)):
        with pytest.raises(ValueError, match="TSDFVolume.find_planes"):
            vol.find_planes(**bad)
    with pytest.raises(ValueError, match="no TSDFVolume"):
        TP.find_planes(types.SimpleNamespace(tsdf=None))
    floor = plane([0, -1, 0], -1.2, 100)
    for bad in (dict(), dict(up_hint=[0, 0, 0]), dict(up_hint=[0, -1, 0], bins=7), dict(plane=floor, heading="north"),
                dict(plane=floor, up_axis=4), dict(plane=floor, up_sign=2), dict(plane=floor, voxel_size=0.0),
                dict(plane={"normal": [0, 0, 3.0], "offset": 0.0}), dict(plane=floor, heading="walls", cone_deg=-1)):
        with pytest.raises(ValueError, match="TSDFVolume.upright"):
            vol.upright(**bad)


# ---- the tilted world -----------------------------------------------------------------------------------------------------
def test_the_restated_pipeline_recovers_the_wall_and_the_floor(tilted):
    """Each plane within atan(voxel / L) of the truth, L the shorter observed side of the plane (a plane whose points err by
    less than half a voxel cannot tilt more), its offset within one voxel, and `floor_plane` under the tilted -y picks
    the floor."""
    vol, planes = tilted["vol"], tilted["planes"]
    print(TP.planes_text(planes))
    assert len(planes) == 2
    found = {}
    for name, (n, o) in tilted["truth"].items():
        best = max(planes, key=lambda p: float(p["normal"] @ n))
        L = shorter_side(plane_points(vol, n, o), n)
        ang = math.degrees(math.acos(min(1.0, float(best["normal"] @ n))))
        print(f"{name}: {best['count']} samples, shorter side {L:.3f} m, angle {ang:.4f} deg against "
              f"{math.degrees(math.atan(VOXEL / L)):.3f}, offset error {best['offset'] - o:+.5f} m, rmse {best['rmse_m']:.5f} m")
        assert L > 0.5 and ang <= math.degrees(math.atan(VOXEL / L))
        assert abs(best["offset"] - o) <= VOXEL and best["rmse_m"] < 0.5 * VOXEL and best["count"] >= 64
        assert abs(best["normal"] @ best["centroid"] - best["offset"]) < 1e-9
        assert best["area_m2"] == best["count"] * VOXEL ** 2 / np.abs(best["normal"]).sum()
        found[name] = best
    assert found["wall"] is planes[0] and found["floor"] is planes[1]             # by descending count
    assert TP.floor_plane(planes, tilted["up"]) is found["floor"]
    assert TP.wall_plane(planes, found["floor"]) is found["wall"]
    assert TP.floor_plane(planes, -tilted["up"]) is None
    again = PR.find_planes(vol, CHUNK)
    assert TP.planes_text(again) == TP.planes_text(planes)


def test_only_the_upright_volume_has_a_level_slab(tilted):
    """The feature: the slab 0.2 .. 1.0 m above the floor.  Upright (up_axis 2, the floor at 0) it shows no column of the
    floor's area occupied and the wall as one straight band; along any lattice axis of the tilted volume it cuts through
    the floor, which fills more than a third of the floor's own columns."""
    vol, planes = tilted["vol"], tilted["planes"]
    floor, wall = planes[1], planes[0]
    for axis in range(3):
        share, n = tilted_slab_share(vol, floor, wall, axis)
        print(f"tilted, lattice axis {axis}: {share:.3f} of {n} floor columns occupied")
        assert n > 50 and share > 1 / 3
    T = TP.upright_transform(floor, 2, 1, wall)
    up = PR.upright(vol, T)
    pts = floor_area_points(vol, floor, wall) @ T[:3, :3].T + T[:3, 3]
    print("the floor's points in the map frame: up coordinate", pts[:, 2].min(), "..", pts[:, 2].max())
    assert np.abs(pts[:, 2]).max() < 0.5 * VOXEL
    cells = slab_cells(up, 2, *SLAB)
    assert_upright_map(cells, footprint(up["lo"], up["tsdf"].shape, VOXEL, pts, 2))
    h = T[:3, :3] @ wall["normal"]
    assert abs(h[0]) < 1e-12 and abs(abs(h[1]) - 1) < 1e-3      # the band runs along the map's first axis
