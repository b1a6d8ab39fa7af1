"""TSDF fusion on the MI355X (csrc/tsdf.hip, go_slam_amd/tsdf.py): the integration kernel equals the serial restatement
(tests/tsdf_restatement.py) bit for bit however the frames are cut into calls, the frustum skip changes nothing, the mesh
equals the restated pipeline, a fronto-parallel plane is recovered to fp32 rounding, an oblique scene to the fp64
restatement's own error, fuse_keyframes feeds the volume what its sources document, and a whole only-tracking run ends
with a coloured mesh/tsdf_mesh.ply."""
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
import tsdf_restatement as TR                                  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

VOXEL = 0.125                                                  # exact in binary: the lattice sizes below are exact
BOUND_EXACT = [[-1.5, 3.0], [-0.75, 1.75], [-2.0, 6.625]]      # 37 x 21 x 70
H, W = 48, 64
INTR = (0.9 * W, 0.9 * W, W / 2 - 0.5, H / 2 - 0.5)


def bits(t):
    t = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t
    return np.ascontiguousarray(t, dtype=np.float32).view(np.int32)


def assert_state(vol, ref):
    assert np.array_equal(bits(vol.weight), bits(ref["weight"]))
    assert np.array_equal(bits(vol.tsdf), bits(ref["tsdf"]))
    assert np.array_equal(bits(vol.colors), bits(ref["colors"]))


def batch():
    from go_slam_amd import _lib
    return int(_lib.lib().gs_tsdf_batch())


def volume(bound=BOUND_EXACT, voxel=VOXEL, **kw):
    from go_slam_amd.tsdf import TSDFVolume
    return TSDFVolume(bound, voxel, device=DEV, **kw)


def restate(frames, dims, lo, voxel, trunc, max_weight=64.0, images=True, vol=None):
    depth, mats, img, mask = frames
    vol = TR.new_volume(dims) if vol is None else vol
    return TR.integrate(vol, depth, mats, INTR, lo, voxel, trunc, max_weight, images=img if images else None, mask=mask)


@pytest.fixture(scope="module")
def arc_frames(built_lib):
    """2 * batch + 1 frames on synth's arc over its wall and floor: 5 % zero depth, a random mask, random colours."""
    from go_slam_amd.tsdf import w2c_matrices
    K = 2 * batch() + 1
    poses = synth.arc_poses(K)
    disp = synth.plane_disps(poses, torch.tensor(INTR), H, W)
    depth = torch.where(disp > 0, 1.0 / disp, torch.zeros_like(disp))
    g = torch.Generator().manual_seed(7)
    depth[torch.rand(K, H, W, generator=g) < 0.05] = 0.0
    mask = (torch.rand(K, H, W, generator=g) > 0.2).float()
    images = torch.rand(K, 3, H, W, generator=g)
    return depth.numpy(), w2c_matrices(poses).numpy(), images.numpy(), mask.numpy()


@pytest.fixture(scope="module")
def arc_reference(arc_frames):
    dims, lo = (37, 21, 70), [b[0] for b in BOUND_EXACT]
    return {mw: restate(arc_frames, dims, lo, VOXEL, 4 * VOXEL, mw) for mw in (64.0, 3.0)}


def integrate(vol, frames, lo=0, hi=None, images=True):
    depth, mats, img, mask = frames
    sl = slice(lo, hi)
    vol.integrate(torch.from_numpy(depth[sl]), torch.from_numpy(mats[sl]), INTR,
                  images=torch.from_numpy(img[sl]) if images else None, mask=torch.from_numpy(mask[sl]))
    return vol


def test_integrate_is_the_restatement_bit_for_bit(arc_frames, arc_reference):
    vol = volume()
    assert vol.dims == (37, 21, 70) and vol.trunc == 0.5
    integrate(vol, arc_frames)
    ref = arc_reference[64.0]
    seen = ref["weight"] > 0
    behind = ref["weight"][:, :, :8] == 0                      # z < -1: behind every camera of the arc
    print("share of points updated:", seen.mean(), "largest weight:", ref["weight"].max())
    assert 0.05 < seen.mean() < 0.9 and behind.all() and ref["weight"].max() > batch()
    assert_state(vol, ref)
    vol.reset()
    assert bool((vol.tsdf == 1).all()) and not bool(vol.weight.any()) and not bool(vol.colors.any())


def test_two_calls_split_at_an_odd_frame_give_the_same_bits(arc_frames, arc_reference):
    vol = volume()
    integrate(vol, arc_frames, 0, 7)
    integrate(vol, arc_frames, 7, None)
    assert_state(vol, arc_reference[64.0])


def test_max_weight_three_is_bit_exact(arc_frames, arc_reference):
    vol = integrate(volume(max_weight=3.0), arc_frames)
    assert float(vol.weight.max()) == 3.0
    assert_state(vol, arc_reference[3.0])


def test_without_images_the_colours_stay_untouched(arc_frames, arc_reference):
    vol = integrate(volume(), arc_frames, images=False)
    ref = arc_reference[64.0]
    assert np.array_equal(bits(vol.tsdf), bits(ref["tsdf"])) and np.array_equal(bits(vol.weight), bits(ref["weight"]))
    assert not bool(vol.colors.any())


def test_bad_lattice_is_refused_before_any_launch(built_lib):
    from go_slam_amd import _lib
    L = _lib.lib()
    x = torch.full((8,), 7.0, device=DEV)
    for dims in [(1, 2, 2), (2, 1025, 2), (2, 2, 0)]:
        rc = L.gs_tsdf_integrate(_lib.ptr(x), _lib.ptr(x), _lib.ptr(x), *dims, _lib.ptr(x), None, None, _lib.ptr(x), 0,
                                 2, 2, 1.0, 1.0, 0.5, 0.5, 0.0, 0.0, 0.0, 0.1, 0.4, 64.0, _lib.stream_ptr(DEV))
        assert rc == -1 and b"outside [2, 1024]" in L.gs_last_error()
    torch.cuda.synchronize()
    assert bool((x == 7.0).all())


def one_frame(R_w2c, centre, depth_value):
    m = np.zeros((1, 3, 4), np.float32)
    m[0, :, :3] = R_w2c
    m[0, :, 3] = -np.asarray(R_w2c, np.float64) @ np.asarray(centre, np.float64)
    g = np.random.default_rng(3)
    return (np.full((1, H, W), depth_value, np.float32), m, g.random((1, 3, H, W), dtype=np.float32),
            np.ones((1, H, W), np.float32))


def test_a_frame_that_looks_away_changes_nothing(arc_frames, arc_reference):
    vol = integrate(volume(), arc_frames)
    before = [bits(t).copy() for t in (vol.tsdf, vol.weight, vol.colors)]
    away = one_frame(np.diag([-1.0, 1.0, -1.0]), (0.75, 0.5, -3.0), 2.0)          # half a turn about y, behind the lattice
    integrate(vol, away)
    for b, t in zip(before, (vol.tsdf, vol.weight, vol.colors)):
        assert np.array_equal(b, bits(t))
    ref = {k: v.copy() for k, v in arc_reference[64.0].items()}
    restate(away, (37, 21, 70), [b[0] for b in BOUND_EXACT], VOXEL, 4 * VOXEL, vol=ref)
    assert np.array_equal(bits(ref["weight"]), before[1])


def test_a_frustum_that_touches_one_corner_updates_the_restatements_points(built_lib):
    corner = one_frame(np.eye(3), (2.6, 1.4, 5.5), 0.8)
    vol = integrate(volume(), corner)
    ref = restate(corner, (37, 21, 70), [b[0] for b in BOUND_EXACT], VOXEL, 4 * VOXEL)
    touched = ref["weight"] > 0
    print("points touched:", int(touched.sum()), "of", touched.size)
    assert 0 < touched.sum() < 0.02 * touched.size
    i, j, k = np.nonzero(touched)
    assert i.min() >= 24 and j.min() >= 10 and k.min() >= 60           # the far corner block only
    assert_state(vol, ref)


# ---- mesh -----------------------------------------------------------------------------------------------------------
BOUND_MESH = [[-2.4375, 2.4375], [-1.6875, 1.6875], [0.0, 4.375]]      # 40 x 28 x 36
PLANE_C = 3.04


def look(yaw_deg, pitch_deg, centre):
    """(camera-to-world rotation, centre) of a camera turned by yaw about y, then pitch about its x."""
    a, b = math.radians(yaw_deg), math.radians(pitch_deg)
    Ry = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
    Rx = np.array([[1, 0, 0], [0, math.cos(b), -math.sin(b)], [0, math.sin(b), math.cos(b)]])
    return Ry @ Rx, np.asarray(centre, np.float64)


def plane_frames(cams, c, seed=5):
    """z-depth of the plane z = c through each camera's pixel centres (float64, rounded once), random colours."""
    fx, fy, cx, cy = INTR
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    ray = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1)
    depth, mats = [], []
    for R, q in cams:
        depth.append((c - q[2]) / (ray @ R.T)[..., 2])
        mats.append(np.concatenate([R.T, (-R.T @ q)[:, None]], 1))
    g = np.random.default_rng(seed)
    return (np.stack(depth).astype(np.float32), np.stack(mats).astype(np.float32),
            g.random((len(cams), 3, H, W), dtype=np.float32), np.ones((len(cams), H, W), np.float32))


@pytest.fixture(scope="module")
def plane_mesh_case(built_lib):
    cams = [look(0, 0, (0, 0, 0.1)), look(12, -5, (-0.5, 0.1, 0.3)), look(-15, 6, (0.6, -0.2, 0.0)),
            look(4, 9, (0.1, -0.4, 0.5))]
    frames = plane_frames(cams, PLANE_C)
    vol = integrate(volume(BOUND_MESH), frames)
    assert vol.dims == (40, 28, 36)
    ref = restate(frames, vol.dims, [b[0] for b in BOUND_MESH], VOXEL, 4 * VOXEL)
    return vol, ref


def test_extract_mesh_is_the_restated_pipeline(plane_mesh_case):
    vol, ref = plane_mesh_case
    assert_state(vol, ref)
    lo = [b[0] for b in BOUND_MESH]
    for min_weight in (1.0, 2.0, 0.0):
        mesh = vol.extract_mesh(min_weight)
        rv, rf, rc = TR.extract_mesh(ref, lo, VOXEL, min_weight)
        assert len(rf) > 100
        assert mesh.vertices.dtype == np.float64 and np.array_equal(mesh.vertices, rv)      # bit for bit
        assert np.array_equal(mesh.faces, rf)
        assert mesh.vertex_colors.dtype == np.uint8 and np.array_equal(mesh.vertex_colors, rc)


def test_kept_vertices_sit_between_observed_points_and_the_back_sheet_is_gone(plane_mesh_case):
    vol, _ = plane_mesh_case
    lo = np.array([b[0] for b in BOUND_MESH])
    weight = vol.weight.cpu().numpy()
    mesh = vol.extract_mesh()
    idx = (mesh.vertices - lo) / VOXEL                       # exact: the voxel is a power of two
    a, b = np.floor(idx).astype(int), np.ceil(idx).astype(int)
    assert (weight[a[:, 0], a[:, 1], a[:, 2]] >= 1).all() and (weight[b[:, 0], b[:, 1], b[:, 2]] >= 1).all()
    assert len(mesh.faces) > 100 and mesh.vertices[:, 2].max() <= PLANE_C + vol.trunc + VOXEL
    assert len(np.unique(mesh.vertex_colors, axis=0)) > 50
    sheet = vol.extract_mesh(min_weight=0.0)
    assert len(sheet.faces) > len(mesh.faces)
    assert len(volume(BOUND_MESH).extract_mesh().faces) == 0          # an empty volume gives an empty mesh


@pytest.mark.parametrize("c", [2.013, 2.0])
def test_fronto_parallel_plane_is_recovered(built_lib, c):
    """The zero crossing of a linear profile is exact up to a handful of fp32 roundings of values <= 4; 1e-5 m is about
    40 ulps at 2 m.  c = 2.0 lies on a lattice plane: the surface must still come out, without NaN."""
    depth, w2c = TR.plane_scene(c)
    vol = volume(TR.PLANE_BOUND, TR.PLANE_VOXEL)
    assert vol.dims == TR.lattice_dims(TR.PLANE_BOUND, TR.PLANE_VOXEL)
    vol.integrate(torch.from_numpy(depth), torch.from_numpy(w2c), TR.PLANE_INTR)
    mesh = vol.extract_mesh()
    assert len(mesh.faces) > 500 and np.isfinite(mesh.vertices).all()
    err = np.abs(mesh.vertices[:, 2] - c).max()
    print(f"c = {c}: {len(mesh.vertices)} vertices, max |z - c| = {err:.3e}")
    assert err <= 1e-5
    tri = mesh.vertices[mesh.faces]
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    if c == 2.013:
        assert (n[:, 2] < 0).all()                          # toward the cameras, which look along +z
    else:
        assert (n[:, 2] < 0).sum() > 500


OBLIQUE_FP64_MAX = 0.026337051391601696     # metres; measured as test_oblique_wall_and_floor's docstring says


def surface_distance(vertices):
    return np.minimum(np.abs(vertices[:, 2] - 4.0), np.abs(vertices[:, 1] - 1.2))


def oblique_inputs():
    seq = synth.PlaneSequence(16, 64, 96, 0.9 * 96, 0.9 * 96, 96 / 2 - 0.5, 64 / 2 - 0.5)
    w2c = torch.linalg.inv(seq.c2w.double())[:, :3, :].float()
    return seq.depths, w2c, seq.intrinsic.tolist(), seq.images


def test_oblique_wall_and_floor(built_lib):
    """synth.PlaneSequence's wall z = 4 and floor y = 1.2 from its 16 ground-truth poses, voxel 0.05.  The largest
    distance of a mesh vertex to the nearer plane, measured once on the float64 restatement (tsdf_restatement.integrate
    with dtype=np.float64, then extract_mesh): 0.02634 m over 10478 vertices (mean 0.00067 m), OBLIQUE_FP64_MAX.  fp32 against fp64 only moves vertices by
    roundings, so the GPU mesh is held to that value plus 10 %."""
    depth, w2c, intr, images = oblique_inputs()
    vol = volume([[-4, 4], [-3, 2], [-1, 5]], 0.05)
    vol.integrate(depth, w2c, intr, images=images)
    mesh = vol.extract_mesh()
    d = surface_distance(mesh.vertices)
    print(f"{len(mesh.vertices)} vertices, max distance {d.max():.5f} m, mean {d.mean():.5f} m")
    assert len(mesh.faces) > 10000
    assert OBLIQUE_FP64_MAX <= 0.05                          # within one voxel, or the scene is wrong
    assert d.max() <= 1.1 * OBLIQUE_FP64_MAX


# ---- fuse_keyframes -------------------------------------------------------------------------------------------------
BOUND_VIDEO = [[-3.0, 3.0], [-2.0, 1.5], [0.0, 5.0]]


def make_video(n_kf, buffer, shape="S480", seed=43):
    """tests/test_pointcloud_gpu.py's video: synth poses, the planes' inverse depth, random RGB."""
    from go_slam_amd.depth_video import DepthVideo
    h8, w8, _ = synth.SHAPES[shape]
    v = DepthVideo(h8, w8, buffer=buffer, device=DEV, full_res=True)
    syn = synth.make_video(n_kf, shape, seed=seed, buffer=buffer)
    v.poses[:] = syn["poses"].to(DEV)
    v.intrinsics[:] = syn["intrinsics"].to(DEV)
    v.disps_up[:n_kf] = synth.plane_disps(v.poses[:n_kf], v.intrinsics[0] * 8, v.ht, v.wd)
    g = torch.Generator(device=DEV).manual_seed(seed)
    v.images.copy_(torch.rand(v.images.shape, generator=g, device=DEV))
    v.counter = n_kf
    return v


def assert_same_volume(a, b):
    for x, y in ((a.tsdf, b.tsdf), (a.weight, b.weight), (a.colors, b.colors)):
        assert np.array_equal(bits(x), bits(y))


def assert_same_mesh(a, b):
    assert len(a.faces) > 100
    assert np.array_equal(a.vertices, b.vertices) and np.array_equal(a.faces, b.faces)
    assert np.array_equal(a.vertex_colors, b.vertex_colors)


def inverse(disp):
    return torch.where(disp > 0, 1.0 / disp, torch.zeros_like(disp))


def test_fuse_keyframes_tracked_is_the_point_clouds_rule(built_lib, monkeypatch):
    import pointcloud_restatement as R
    from go_slam_amd import tsdf
    v = make_video(12, 16)
    intr = (v.intrinsics[0] * 8).contiguous()
    index = [0, 1, 2, 4, 5, 7, 8, 9, 10, 11]
    monkeypatch.setattr(tsdf, "CHUNK", 4)                    # three chunks
    vol, mesh = tsdf.fuse_keyframes(v, BOUND_VIDEO, 0.1, source="tracked", index=index)
    ix = torch.tensor(index, device=DEV)
    disps = v.disps_up[ix]
    count = R.tracked_counts(v.poses, v.disps_up, intr, index, 0.01)
    mask = ((count >= 2) & (disps > 0.01 * disps.mean(dim=[1, 2], keepdim=True))).float()
    assert 0.1 < float(mask.mean()) < 1.0
    hand = volume(BOUND_VIDEO, 0.1)
    hand.integrate(inverse(disps), v.poses[ix], intr.cpu().tolist(), images=v.images[ix], mask=mask)
    assert_same_volume(vol, hand)
    assert_same_mesh(mesh, hand.extract_mesh())
    every, _ = tsdf.fuse_keyframes(v, BOUND_VIDEO, 0.1)      # default: all keyframes below the counter
    assert float(every.weight.sum()) > float(vol.weight.sum())


def test_fuse_keyframes_filtered_follows_pose_compensate(built_lib):
    import go_slam_amd.multiview_filter as MV
    from go_slam_amd import tsdf
    from go_slam_amd.lietorch_shim import SE3
    v = make_video(12, 16)
    cfg = {"tracking": {"warmup": 8, "multiview_filter": {"thresh": 0.01, "visible_num": 2, "kernel_size": 3,
                                                          "bound_enlarge_scale": 1.1}}}
    slam = types.SimpleNamespace(net=None, video=v, verbose=False, mode="rgbd")
    MV.MultiviewFilter(cfg, types.SimpleNamespace(device=DEV), slam)()
    f = int(v.filtered_id[0])
    assert f == 12
    intr = (v.intrinsics[0] * 8).contiguous().cpu().tolist()
    comp = torch.tensor([0.1, -0.2, 0.05, 0.0, 0.0, 0.0998334, 0.9950042], device=DEV)
    meshes = {}
    for name, pc in (("identity", v.pose_compensate[0].clone()), ("moved", comp)):
        v.pose_compensate[0] = pc
        vol, mesh = tsdf.fuse_keyframes(v, BOUND_VIDEO, 0.1, source="filtered")
        w2c = (SE3(v.poses_filtered[:f]) * SE3(pc.clone().unsqueeze(0)).inv()).data
        hand = volume(BOUND_VIDEO, 0.1)
        hand.integrate(inverse(v.disps_filtered[:f]), w2c, intr, images=v.images[:f], mask=v.mask_filtered[:f])
        assert_same_volume(vol, hand)
        assert_same_mesh(mesh, hand.extract_mesh())
        meshes[name] = mesh
    # the moved mesh is the scene carried by w2w: brought back by its inverse, its vertices lie on the wall and the floor
    # again (the median vertex within half a voxel: depth is looked up at the nearest pixel and the filter keeps
    # disparities that agree to its threshold), while in place they do not
    M = SE3(comp.double().cpu().unsqueeze(0)).matrix()[0].numpy()
    moved = meshes["moved"].vertices
    back = (moved - M[:3, 3]) @ M[:3, :3]
    d_id, d_back = np.median(surface_distance(meshes["identity"].vertices)), np.median(surface_distance(back))
    floor = (np.abs(back[:, 1] - 1.2) < 0.05) & (np.abs(back[:, 2] - 4.0) > 0.3)
    d_moved = np.median(np.abs(moved[floor, 1] - 1.2))      # w2w tilts the floor by 11 degrees and lifts it by 0.2 m
    print(f"median distance to the planes: identity {d_id:.4f}, moved and brought back {d_back:.4f}; "
          f"{floor.sum()} floor vertices, in place {d_moved:.4f} from y = 1.2")
    assert d_id < 0.05 and d_back < 0.05 and floor.sum() > 100 and d_moved > 0.1


# ---- a whole run ----------------------------------------------------------------------------------------------------
N_RUN, H_RUN, W_RUN = 16, 64, 96


def make_cfg(out_dir, only_tracking):
    """tests/test_slam_gpu.py's configuration."""
    dev = "cuda:0"
    Hh, Ww = H_RUN, W_RUN
    return {
        "sync_method": "strict", "verbose": False, "dataset": "synthetic", "mode": "rgbd", "stride": 1,
        "only_tracking": only_tracking,
        "mapping": {"device": dev, "BA": False, "BA_cam_lr": 0.001, "net_lr": 0.001, "grid_lr": 0.01,
                    "w_color_loss": 2.0, "w_sdf_smooth_loss": 1.0, "w_sdf_loss": 2.0, "w_eikonal_loss": 0.1,
                    "uncertainty_weight_loss": True, "mapping_window_size": 22, "pixels": 512, "iters": 2,
                    "post_processing_iters": 2, "decay": 0.8, "bound": [[-4.0, 4.0], [-3.0, 2.0], [-1.0, 5.0]],
                    "model": {"sdf_smooth_std": 0.005, "sdf_sparse_factor": 5, "sdf_truncation": 0.16,
                              "sdf_random_weight": 0.04, "sdf_network": {"d_in": 3, "d_out": 32},
                              "color_network": {"d_in": 3, "d_feat": 31, "d_hidden": 64, "n_layers": 2},
                              "variance_network": {"init_val": 0.2, "scale_factor": 10.0}}},
        "tracking": {"device": dev, "pretrained": None, "buffer": 32, "beta": 0.75, "warmup": 8, "upsample": True,
                     "motion_filter": {"thresh": 0.0},
                     "multiview_filter": {"thresh": 0.05, "visible_num": 2, "kernel_size": 1, "bound_enlarge_scale": 1.10},
                     "frontend": {"enable_loop": True, "keyframe_thresh": 0.0, "thresh": 1e4, "window": 25, "radius": 1,
                                  "nms": 1, "max_factors": 75},
                     "backend": {"thresh": 1e4, "radius": 1, "nms": 5, "loop_window": 25, "loop_thresh": 1e4,
                                 "loop_radius": 1, "loop_nms": 12}},
        "cam": {"H": Hh, "W": Ww, "fx": 0.9 * Ww, "fy": 0.9 * Ww, "cx": Ww / 2 - 0.5, "cy": Hh / 2 - 0.5,
                "png_depth_scale": 1000.0, "calibration_txt": "", "H_edge": 0, "W_edge": 0, "H_out": Hh, "W_out": Ww},
        "rendering": {"N_samples": 24, "N_surface": 48, "lindisp": False, "perturb": 1.0},
        "data": {"input_folder": "synthetic", "output": out_dir, "video_length": ""},
        "meshing": {"level_set": 0, "resolution": 32, "eval_rec": False, "get_largest_components": False,
                    "remove_small_geometry_threshold": 0.2, "n_points_to_eval": 200000, "mesh_threshold_to_eval": 0.05,
                    "gt_mesh_path": "", "forecast_radius": 0},
    }


def whole_run(out_dir, tsdf_cfg):
    from go_slam_amd.slam import SLAM
    import random
    torch.manual_seed(43)
    torch.cuda.manual_seed_all(43)
    np.random.seed(43)
    random.seed(43)
    cfg = make_cfg(out_dir, True)
    if tsdf_cfg is not None:
        cfg["tsdf"] = tsdf_cfg
    args = types.SimpleNamespace(device="cuda:0", make_video=False, output=None)
    slam = SLAM(args, cfg, full_ba_every=4)
    with torch.no_grad():       # small output heads: a random network must not throw the poses to infinity
        slam.net.update.delta[2].weight.mul_(0.02)
        slam.net.update.delta[2].bias.zero_()
    slam.ba.frontend_window = 8
    stream = synth.PlaneSequence(N_RUN, H_RUN, W_RUN, 0.9 * W_RUN, 0.9 * W_RUN, W_RUN / 2 - 0.5, H_RUN / 2 - 0.5)
    slam.run(stream)
    slam.terminate(rank=-1, stream=stream)
    torch.cuda.synchronize()
    return slam


def listing(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_only_tracking_run_ends_with_a_coloured_tsdf_mesh(built_lib, tmp_path):
    from go_slam_amd.neus.mesh import load_mesh
    with_dir, without_dir = str(tmp_path / "with"), str(tmp_path / "without")
    whole_run(with_dir, {"enable": True, "source": "sensor", "voxel_size": 0.1})
    mesh = load_mesh(f"{with_dir}/mesh/tsdf_mesh.ply")
    print(f"{len(mesh.vertices)} vertices, {len(mesh.faces)} faces, extent {mesh.vertices.min(0)} .. {mesh.vertices.max(0)}")
    assert mesh.vertex_colors is not None and len(mesh.faces) >= 1
    assert len(mesh.vertex_colors) == len(mesh.vertices) and len(np.unique(mesh.vertex_colors, axis=0)) > 1
    bound = np.array([[-4.0, 4.0], [-3.0, 2.0], [-1.0, 5.0]])
    assert (mesh.vertices >= bound[:, 0]).all() and (mesh.vertices <= bound[:, 1]).all()
    whole_run(without_dir, None)
    a, b = (np.load(f"{d}/checkpoints/est_poses.npy") for d in (with_dir, without_dir))
    print("files with:", listing(with_dir), "without:", listing(without_dir), "largest pose difference:", np.abs(a - b).max())
    assert not os.path.exists(f"{without_dir}/mesh/tsdf_mesh.ply")      # (the directory itself is Mesher.__init__'s)
    assert [p for p in listing(with_dir) if p != os.path.join("mesh", "tsdf_mesh.ply")] == listing(without_dir)
    assert np.array_equal(np.load(f"{with_dir}/checkpoints/est_poses.npy"),
                          np.load(f"{without_dir}/checkpoints/est_poses.npy"))
    assert open(f"{with_dir}/metrics_traj.txt").read() == open(f"{without_dir}/metrics_traj.txt").read()
