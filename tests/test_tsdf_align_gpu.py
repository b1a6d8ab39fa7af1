"""SDF pose alignment on the MI355X (csrc/tsdf_align.hip, go_slam_amd/localize.py): the Gauss-Newton rows, the step, a
whole `align` and its trace equal tests/tsdf_align_restatement.py bit for bit (int64 views of the doubles) at every
stride, across chunk boundaries and for every input the contract names; bad arguments are refused without a write;
`relocalize` finds the displaced true pose among 32 candidates; a saved volume aligns like the original; and an
only-tracking rgbd run with tsdf.align ends with metrics_tsdf_align.txt and a loadable volume."""
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from go_slam_amd import synth                                  # noqa: E402
import test_tsdf_gpu as TG                                     # noqa: E402  (its lattice, frames and whole run)
import test_tsdf_raycast_cpu as RC                             # noqa: E402  (look, cam)
import tsdf_align_restatement as AR                            # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W = TG.H, TG.W
LO = [b[0] for b in TG.BOUND_EXACT]
GUARD = 64                                                     # doubles of padding on each side of a guarded buffer


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def chunk():
    from go_slam_amd import _lib
    return int(_lib.lib().gs_tsdf_align_chunk())


def c2w_of(w2c7):
    from go_slam_amd.lietorch_shim import SE3
    return SE3(w2c7.double()).inv().matrix().numpy()[:, :3, :]


def raw_system(vol, depth, frame, pose, stride, intr, max_depth=math.inf, min_weight=1.0, huber=0.5, k=None):
    """gs_tsdf_align_system through ctypes on fresh buffers -> (rc, rows [B,32] host)."""
    from go_slam_amd import _lib
    L = _lib.lib()
    depth_d = torch.as_tensor(depth, dtype=torch.float32).to(DEV).contiguous()
    kk, h, w = depth_d.shape
    B = len(frame)
    frame_d = torch.as_tensor(np.asarray(frame, np.int32)).to(DEV)
    pose_d = torch.as_tensor(np.asarray(pose, np.float64).reshape(B, 3, 4)).to(DEV).contiguous()
    ws = torch.empty(max(L.gs_tsdf_align_workspace_bytes(B, h, w, stride) // 8, 1), dtype=torch.float64, device=DEV)
    out = torch.full((B, 32), 7.0, dtype=torch.float64, device=DEV)
    nx, ny, nz = vol.dims
    rc = L.gs_tsdf_align_system(_lib.ptr(vol.tsdf), _lib.ptr(vol.weight), nx, ny, nz, _lib.ptr(depth_d), _lib.ptr(frame_d),
                                _lib.ptr(pose_d), B, kk if k is None else k, h, w, stride, *intr, float(vol.lo[0]),
                                float(vol.lo[1]), float(vol.lo[2]), vol.voxel, max_depth, min_weight, huber, _lib.ptr(ws),
                                _lib.ptr(out), _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()


def restated(scene, depth, frame, pose, stride, intr, **kw):
    return AR.system(scene["tsdf"], scene["weight"], np.asarray(depth, np.float32), frame, pose, stride, intr, LO, TG.VOXEL,
                     chunk(), **kw)


@pytest.fixture(scope="module")
def scene(built_lib):
    """test_tsdf_gpu.py's 37 x 21 x 70 lattice fused on the GPU from its arc frames (5 % zero depth, a random mask: real
    weights and unseen cells); three of the depth maps, the third with NaN and negative pixels; six float64 poses: three
    of the arc, moved a little off their truth, one outside the box looking in, one with identity rotation, one looking
    away."""
    K = 2 * TG.batch() + 1
    poses = synth.arc_poses(K)
    disp = synth.plane_disps(poses, torch.tensor(TG.INTR), H, W)
    depth = torch.where(disp > 0, 1.0 / disp, torch.zeros_like(disp))
    g = torch.Generator().manual_seed(7)
    depth[torch.rand(K, H, W, generator=g) < 0.05] = 0.0
    mask = (torch.rand(K, H, W, generator=g) > 0.2).float()
    images = torch.rand(K, 3, H, W, generator=g)
    vol = TG.volume()
    assert vol.dims == (37, 21, 70)
    vol.integrate(depth, poses, TG.INTR, images=images, mask=mask)
    ids = [0, K // 2, K - 1]
    maps = depth[ids].numpy().copy()
    maps[2, 5:9, 10:30] = np.nan
    maps[2, 20:24, 40:60] = -1.5
    arc = c2w_of(poses[ids])
    rng = np.random.default_rng(11)
    moved = np.stack([AR.displaced(m, 0.03, 1.5, rng) for m in arc])
    extra = np.stack([RC.look(90.0, 0.0, (-2.5, 0.3, 2.0)), RC.cam((0.7, 0.4, -0.5))[0],
                      RC.cam((0.75, 0.5, -3.0), np.diag([-1.0, 1.0, -1.0]))[0]])
    return {"vol": vol, "tsdf": vol.tsdf.cpu().numpy(), "weight": vol.weight.cpu().numpy(), "maps": maps,
            "pose": np.concatenate([moved, extra]), "frame": [0, 1, 2, 0, 1, 2], "arc_w2c": poses, "arc_depth": depth,
            "arc_c2w": c2w_of(poses)}


@pytest.mark.parametrize("stride", [1, 2, 3, 5])
def test_rows_equal_the_restatement_bit_for_bit(scene, stride):
    ref = restated(scene, scene["maps"], scene["frame"], scene["pose"], stride, TG.INTR)
    print("count per pose:", ref[:, 28], "considered:", ref[:, 30])
    assert (ref[:3, 28] > 0).all() and ref[5, 28] == 0 and ref[5, 30] > 0       # looking away: no sample
    assert (ref[:, 31] == 0).all()
    rc, out = raw_system(scene["vol"], scene["maps"], scene["frame"], scene["pose"], stride, TG.INTR)
    assert rc == 0
    assert same_bits(out, ref)


@pytest.mark.parametrize("kw", [dict(min_weight=3.0), dict(huber=0.1), dict(max_depth=3.9), dict(min_weight=3.0, huber=0.1,
                                                                                                   max_depth=3.9)])
def test_thresholds_and_bad_depths_follow_the_restatement(scene, kw):
    """max_depth 3.9 cuts the wall at z = 4 off and keeps the floor; map 2 holds NaN and negative depths."""
    base = restated(scene, scene["maps"], scene["frame"], scene["pose"], 1, TG.INTR)
    ref = restated(scene, scene["maps"], scene["frame"], scene["pose"], 1, TG.INTR, **kw)
    print(kw, "count:", ref[:, 28], "of", base[:, 28])
    assert (ref[:3, 28] > 0).all()
    if "huber" not in kw or len(kw) > 1:
        assert (ref[:3, 28] < base[:3, 28]).all()
    else:
        assert (ref[:3, 28] == base[:3, 28]).all() and (ref[:3, 27] <= base[:3, 27]).all()     # the same samples, down-weighted
    rc, out = raw_system(scene["vol"], scene["maps"], scene["frame"], scene["pose"], 1, TG.INTR, **kw)
    assert rc == 0 and same_bits(out, ref)


def line_case(scene, width):
    """A 1 x width image along the optical centre's row from the first arc pose: the wall at z = 4."""
    intr = (0.9 * width, 0.9 * width, width / 2 - 0.5, 0.0)
    disp = synth.plane_disps(scene["arc_w2c"][:1], torch.tensor(intr), 1, width)
    return torch.where(disp > 0, 1.0 / disp, torch.zeros_like(disp)).numpy(), intr


def test_chunk_boundaries(scene):
    C = chunk()
    assert C in (1024, 2048, 4096)
    pose = scene["arc_c2w"][:1]
    for width in (1, C - 1, C, C + 1):
        depth, intr = line_case(scene, width)
        ref = restated(scene, depth, [0], pose, 1, intr)
        print("width", width, "count", ref[0, 28], "of", ref[0, 30])
        assert ref[0, 30] == width and (width == 1 or ref[0, 28] >= 0.25 * width)
        rc, out = raw_system(scene["vol"], depth, [0], pose, 1, intr)
        assert rc == 0 and same_bits(out, ref)


@pytest.mark.parametrize("B", [1, 8])
def test_several_chunks_and_poses_sharing_a_map(scene, B):
    """96 x 128 at stride 1: 12288 samples, several chunks whatever the chunk size; k = 3 maps, eight poses on them."""
    intr = tuple(2 * v for v in TG.INTR[:2]) + (63.5, 47.5)
    ids = [0, 8, 16]
    disp = synth.plane_disps(scene["arc_w2c"][ids], torch.tensor(intr), 96, 128)
    depth = torch.where(disp > 0, 1.0 / disp, torch.zeros_like(disp)).numpy()
    frame = [0, 0, 1, 2, 2, 1, 0, 2][:B]
    rng = np.random.default_rng(5)
    pose = np.stack([AR.displaced(scene["arc_c2w"][ids[f]], 0.02, 1.0, rng) for f in frame])
    ref = restated(scene, depth, frame, pose, 1, intr)
    assert (ref[:, 28] > 0).all()
    rc, out = raw_system(scene["vol"], depth, frame, pose, 1, intr)
    assert rc == 0 and same_bits(out, ref)
    rc, again = raw_system(scene["vol"], depth, frame, pose, 1, intr)
    assert same_bits(out, again)                                # two runs agree bitwise


def raw_step(rows, pose, lam_rel, lam_abs, min_count):
    from go_slam_amd import _lib
    B = rows.shape[0]
    rows_d = torch.as_tensor(rows).to(DEV).contiguous()
    pose_d = torch.as_tensor(np.asarray(pose, np.float64)).to(DEV).contiguous()
    trace = torch.full((B, 4), 7.0, dtype=torch.float64, device=DEV)
    rc = _lib.lib().gs_tsdf_align_step(_lib.ptr(rows_d), _lib.ptr(pose_d), B, lam_rel, lam_abs, min_count, _lib.ptr(trace),
                                      _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    return rc, pose_d.cpu().numpy(), trace.cpu().numpy()


@pytest.mark.parametrize("lam", [(1e-6, 1e-9, 64), (0.0, 0.0, 1), (1e-6, 1e-9, 100000)])
def test_step_equals_the_restatement(scene, lam):
    """Rows of the fused scene (the look-away pose has count 0) plus a row with samples and a zero H: without lam_abs
    its first pivot fails.  min_count 100000 refuses every row."""
    rows = restated(scene, scene["maps"], scene["frame"], scene["pose"], 2, TG.INTR)
    flat = np.zeros((1, 32))
    flat[0, 28], flat[0, 30] = 500.0, 600.0
    rows = np.concatenate([rows, flat])
    pose = np.concatenate([scene["pose"], scene["pose"][:1]])
    ref_pose, ref_trace = AR.step(rows, pose, *lam)
    print(lam, "status:", ref_trace[:, 3])
    if lam[2] == 64:
        assert ref_trace[:3, 3].tolist() == [1, 1, 1] and ref_trace[5, 3] == 0 and ref_trace[6, 3] == 1
    if lam[2] == 1:
        assert ref_trace[6, 3] == 0 and same_bits(ref_pose[6], pose[6])
    if lam[2] == 100000:
        assert not ref_trace[:, 3].any() and same_bits(ref_pose, pose)
    rc, got_pose, got_trace = raw_step(rows, pose, *lam)
    assert rc == 0
    assert same_bits(got_trace, ref_trace) and same_bits(got_pose, ref_pose)


@pytest.fixture(scope="module")
def room(built_lib, tmp_path_factory):
    """The restatement's three-plane scene, off the lattice, as a TSDFVolume (through save's file format and load)."""
    from go_slam_amd.tsdf import TSDFVolume
    tsdf, weight = AR.scene_volume(AR.PLANES_OFF)
    path = str(tmp_path_factory.mktemp("room") / "room.npz")
    np.savez(path, tsdf=tsdf, weight=weight, colors=np.zeros((3,) + tsdf.shape, np.float32),
             lo=np.asarray(AR.SCENE_LO, np.float64), voxel=np.float64(AR.SCENE_VOXEL), trunc=np.float64(AR.SCENE_TRUNC),
             max_weight=np.float64(64.0), dims=np.asarray(tsdf.shape, np.int64))
    vol = TSDFVolume.load(path, device=DEV)
    truth = AR.scene_pose()
    depth = AR.scene_depth(truth, AR.PLANES_OFF)
    rng = np.random.default_rng(3)
    starts = np.stack([AR.displaced(truth, m, d, rng) for m, d in ((0.05, 3.0), (0.10, 5.0), (0.15, 8.0))])
    return {"vol": vol, "tsdf": tsdf, "weight": weight, "truth": truth, "depth": depth, "starts": starts, "path": path}


def test_align_equals_the_restatement_and_converges(room):
    """Bit equality hands the CPU suite's convergence assertions to the GPU; they are repeated on the GPU's poses."""
    vol = room["vol"]
    ref_pose, ref_rows, ref_trace = AR.align(room["tsdf"], room["weight"], room["depth"][None], [0, 0, 0], room["starts"],
                                             AR.SCENE_INTR, AR.SCENE_LO, AR.SCENE_VOXEL, chunk())
    res = vol.align(room["depth"], room["starts"], AR.SCENE_INTR, frame=[0, 0, 0])
    assert same_bits(res["c2w"][:, :3, :], ref_pose)
    assert same_bits(res["trace"], ref_trace) and res["trace"].shape == (25, 3, 4)
    assert res["ok"].all() and (res["count"] == ref_rows[:, 28]).all()
    assert same_bits(res["rmse_m"], AR.SCENE_TRUNC * np.sqrt(ref_rows[:, 29] / ref_rows[:, 28]))
    errs = [AR.pose_error(p[:3], room["truth"]) for p in res["c2w"]]
    print("errors against the truth (m, deg):", errs, "moved:", res["moved_m"], res["moved_deg"])
    # three planes constrain every direction: the constrained movement is the movement
    assert (res["n_constrained"] == 3).all() and np.abs(res["moved_constrained_m"] - res["moved_m"]).max() <= 1e-15
    assert all(m <= AR.SCENE_VOXEL / 10 and d <= 0.1 for m, d in errs)
    assert max(np.linalg.norm(res["c2w"][i, :3, 3] - res["c2w"][0, :3, 3]) for i in range(3)) <= 1e-5
    again = vol.align(room["depth"], room["starts"], AR.SCENE_INTR, frame=[0, 0, 0])
    assert same_bits(again["c2w"], res["c2w"]) and same_bits(again["trace"], res["trace"])
    scores = vol.pose_scores(room["depth"], res["c2w"], AR.SCENE_INTR, frame=[0, 0, 0], stride=1)
    assert same_bits(scores["rmse_m"], res["rmse_m"]) and (scores["count"] == res["count"]).all()


def test_saved_volume_aligns_like_the_original(room, tmp_path):
    from go_slam_amd.tsdf import TSDFVolume
    vol = room["vol"]
    path = str(tmp_path / "v.npz")
    vol.save(path)
    back = TSDFVolume.load(path, device=DEV)
    assert back.dims == vol.dims and back.voxel == vol.voxel and back.trunc == vol.trunc
    assert np.array_equal(back.lo, vol.lo) and back.max_weight == vol.max_weight
    for a, b in ((back.tsdf, vol.tsdf), (back.weight, vol.weight), (back.colors, vol.colors)):
        assert np.array_equal(TG.bits(a), TG.bits(b))
    one = vol.align(room["depth"], room["starts"][:1], AR.SCENE_INTR)
    two = back.align(room["depth"], room["starts"][:1], AR.SCENE_INTR)
    assert same_bits(one["c2w"], two["c2w"]) and same_bits(one["trace"], two["trace"])


def test_bad_arguments_are_refused_without_a_write(scene):
    """Every refusal of the C ABI returns GS_ERR_INVALID_ARG (-1) before a launch: out, pose and workspace, each between
    guard bands, keep their fill.  An out-of-range frame entry is the device's to catch: a zero row."""
    from go_slam_amd import _lib
    L = _lib.lib()
    vol = scene["vol"]
    nx, ny, nz = vol.dims
    depth = torch.as_tensor(scene["maps"]).to(DEV).contiguous()
    frame = torch.zeros(2, dtype=torch.int32, device=DEV)
    fill = 7.0
    n_ws = L.gs_tsdf_align_workspace_bytes(2, H, W, 1) // 8
    out = torch.full((2 * GUARD + 64,), fill, dtype=torch.float64, device=DEV)
    pose = torch.full((2 * GUARD + 24,), fill, dtype=torch.float64, device=DEV)
    ws = torch.full((2 * GUARD + n_ws,), fill, dtype=torch.float64, device=DEV)
    pose[GUARD:GUARD + 24] = torch.as_tensor(scene["pose"][:2].reshape(-1)).to(DEV)
    pose_before = pose.clone()
    good = dict(tsdf=vol.tsdf, weight=vol.weight, nx=nx, ny=ny, nz=nz, depth=depth, frame=frame, pose=pose[GUARD:], B=2, k=3,
                h=H, w=W, stride=1, fx=TG.INTR[0], fy=TG.INTR[1], cx=TG.INTR[2], cy=TG.INTR[3], lox=LO[0], loy=LO[1],
                loz=LO[2], voxel=TG.VOXEL, max_depth=math.inf, min_weight=1.0, huber=0.5, ws=ws[GUARD:], out=out[GUARD:])

    def call(**bad):
        a = dict(good, **bad)
        p = {k: (_lib.ptr(v) if isinstance(v, torch.Tensor) or v is None else v) for k, v in a.items()}
        return L.gs_tsdf_align_system(p["tsdf"], p["weight"], p["nx"], p["ny"], p["nz"], p["depth"], p["frame"], p["pose"],
                                      p["B"], p["k"], p["h"], p["w"], p["stride"], p["fx"], p["fy"], p["cx"], p["cy"],
                                      p["lox"], p["loy"], p["loz"], p["voxel"], p["max_depth"], p["min_weight"], p["huber"],
                                      p["ws"], p["out"], _lib.stream_ptr(DEV))

    bads = [dict(nx=1), dict(ny=1025), dict(nz=0), dict(B=-1), dict(k=-1), dict(k=0), dict(h=0), dict(w=0), dict(stride=0),
            dict(stride=-2), dict(fx=0.0), dict(fy=0.0), dict(fx=math.nan), dict(cx=math.inf), dict(voxel=0.0),
            dict(voxel=-0.1), dict(voxel=math.inf), dict(voxel=math.nan), dict(lox=math.nan), dict(huber=0.0),
            dict(huber=-1.0), dict(huber=math.nan), dict(max_depth=0.0), dict(max_depth=math.nan), dict(min_weight=math.nan),
            dict(tsdf=None), dict(weight=None), dict(depth=None), dict(frame=None), dict(pose=None), dict(ws=None),
            dict(out=None)]
    for bad in bads:
        assert call(**bad) == -1, bad
        assert L.gs_last_error().startswith(b"tsdf_align_system"), bad
    step_bads = [dict(B=-1), dict(lam_rel=-1.0), dict(lam_rel=math.nan), dict(lam_abs=math.inf), dict(lam_abs=-1e-9),
                 dict(min_count=0), dict(out=None), dict(pose=None)]
    for bad in step_bads:
        a = dict(dict(out=out[GUARD:], pose=pose[GUARD:], B=2, lam_rel=1e-6, lam_abs=1e-9, min_count=64), **bad)
        rc = L.gs_tsdf_align_step(_lib.ptr(a["out"]), _lib.ptr(a["pose"]), a["B"], a["lam_rel"], a["lam_abs"], a["min_count"],
                                  None, _lib.stream_ptr(DEV))
        assert rc == -1 and L.gs_last_error().startswith(b"tsdf_align_step"), bad
    assert L.gs_tsdf_align_workspace_bytes(-1, H, W, 1) == 0 and L.gs_tsdf_align_workspace_bytes(1, H, W, 0) == 0
    assert L.gs_tsdf_align_workspace_bytes(1, 0, W, 1) == 0 and L.gs_tsdf_align_workspace_bytes(2, H, W, 1) == n_ws * 8
    assert call(B=0) == 0                                       # nothing to do, nothing launched
    torch.cuda.synchronize()
    assert bool((out == fill).all()) and bool((ws == fill).all()) and torch.equal(pose, pose_before)
    # frame values are read on the device: poses 0 and 2 of four point outside [0, 3)
    fr = [-1, 1, 3, 0]
    pose4 = scene["pose"][[0, 1, 2, 0]]
    rc, rows = raw_system(vol, scene["maps"], fr, pose4, 2, TG.INTR)
    ref = restated(scene, scene["maps"], fr, pose4, 2, TG.INTR)
    assert rc == 0 and not rows[0].any() and not rows[2].any() and rows[1, 28] > 0 and same_bits(rows, ref)
    rc, got_pose, trace = raw_step(rows, pose4, 1e-6, 1e-9, 64)
    assert trace[:, 3].tolist() == [0, 1, 0, 1] and same_bits(got_pose[[0, 2]], pose4[[0, 2]])


def test_relocalize_finds_the_displaced_true_pose(scene):
    """4 standpoints x 8 headings about y (the scene's y grows downward).  Standpoint 0 is the centre of arc pose 4 moved
    by 4 cm; its heading 2 looks along +z, 2 degrees off that pose's yaw.  The wall and the floor leave the translation
    along x free, so the result is held to `align` from that candidate, bit for bit, and to the observable part of the
    truth."""
    from go_slam_amd import localize
    vol = scene["vol"]
    truth = scene["arc_c2w"][4]
    depth = scene["arc_depth"][4]
    centres = np.array([truth[:, 3] + np.array([0.0, 0.024, 0.032]), [1.5, -0.3, 1.6], [-0.6, 0.6, 2.4], [0.4, 0.2, -1.2]])
    cand = localize.candidate_poses(centres, 8, 1, up_sign=-1)
    assert cand.shape == (32, 4, 4) and np.allclose(np.linalg.det(cand[:, :3, :3]), 1.0)
    start = AR.pose_error(cand[2, :3], truth)
    print("candidate 2 against the truth (m, deg):", start)
    assert abs(start[0] - 0.04) < 1e-6 and abs(start[1] - 2.0) < 1e-3
    res = localize.relocalize(vol, depth, TG.INTR, cand, keep=8, min_inlier_fraction=0.5)
    print("found", res["found"], "index", res["index"], "rmse", res["rmse_m"], "inliers", res["inlier_fraction"],
          "ranked:", [(r["index"], round(r["rmse_m"], 4), round(r["inlier_fraction"], 3), r["ok"]) for r in res["ranked"]])
    assert res["found"] and res["index"] == 2 and len(res["ranked"]) == 8
    alone = vol.align(depth, cand[2:3], TG.INTR)
    assert same_bits(res["c2w"], alone["c2w"][0]) and alone["ok"][0]
    end = AR.pose_error(res["c2w"][:3], truth)
    print("aligned against the truth (m, deg):", end, "y, z:", res["c2w"][1:3, 3] - truth[1:, 3])
    assert end[1] < start[1]                                    # the wall fixes the yaw: the alignment must not lose ground
    none = localize.relocalize(vol, depth, TG.INTR, cand, keep=8, min_inlier_fraction=1.01)
    assert not none["found"] and len(none["ranked"]) == 8


def test_only_tracking_run_with_align_and_a_saved_volume(built_lib, tmp_path, monkeypatch):
    from go_slam_amd import localize
    from go_slam_amd.slam import SLAM
    from go_slam_amd.tsdf import TSDFVolume
    returned = []
    terminate = SLAM.terminate

    def keeping(self, *args, **kw):
        returned.append(terminate(self, *args, **kw))
        return returned[-1]
    monkeypatch.setattr(SLAM, "terminate", keeping)
    with_dir, without_dir = str(tmp_path / "with"), str(tmp_path / "without")
    base = {"enable": True, "source": "sensor", "voxel_size": 0.1}
    TG.whole_run(with_dir, dict(base, save_volume=True, align={"enable": True, "every": 3, "min_count": 32}))
    text = open(f"{with_dir}/metrics_tsdf_align.txt").read()
    result, frames = localize.parse_align(text)
    print(text)
    assert [f[0] for f in frames] == list(range(0, TG.N_RUN, 3)) and result["n_frames"] == len(frames)
    per_frame = np.array([f[1:] for f in frames], np.float64)
    again = localize.summarize_align(per_frame)
    assert localize.align_text(again, [f[0] for f in frames], per_frame) == text           # the text round trip, bit for bit
    assert result["n_failed"] == int((per_frame[:, 6] == 0).sum()) and result["n_failed"] < len(frames)
    stats = returned[0]
    assert stats["tsdf_align_moved_mean_m"] == result["moved_mean_m"] == per_frame[per_frame[:, 6] == 1, 0].mean()
    assert stats["tsdf_align_moved_max_m"] == result["moved_max_m"] == per_frame[per_frame[:, 6] == 1, 0].max()
    assert stats["tsdf_align_moved_constrained_mean_m"] == result["moved_constrained_mean_m"]
    assert stats["tsdf_align_failed"] == result["n_failed"]
    # the wall and the floor leave the direction along their edge free: two constrained directions in every frame, and
    # the movement along them is a projection of the whole movement
    assert (per_frame[:, 5] == 2).all() and result["n_underconstrained"] == len(frames) - result["n_failed"]
    assert (per_frame[:, 4] <= per_frame[:, 0] * (1 + 1e-12)).all()
    vol = TSDFVolume.load(f"{with_dir}/mesh/tsdf_volume.npz", device=DEV)
    assert len(vol.dims) == 3 and float(vol.weight.max()) >= 1.0 and float(vol.tsdf.min()) < 0
    TG.whole_run(without_dir, base)
    assert not [k for k in returned[1] if "tsdf_align" in k]
    assert set(returned[0]) - set(returned[1]) == {"tsdf_align_moved_mean_m", "tsdf_align_moved_max_m",
                                                   "tsdf_align_moved_constrained_mean_m", "tsdf_align_failed"}
    new = {"metrics_tsdf_align.txt", os.path.join("mesh", "tsdf_volume.npz")}
    assert [p for p in TG.listing(with_dir) if p not in new] == TG.listing(without_dir)
    assert new <= set(TG.listing(with_dir))
