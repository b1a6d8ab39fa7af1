"""The TSDF raycast on the MI355X (csrc/tsdf_raycast.hip, TSDFVolume.raycast): depth, normal, colour and the hit mask
equal the serial restatement (tests/tsdf_raycast_restatement.py) bit for bit at every step length, with and without the
brick skip and however the frames are cut into calls; a plane is recovered from an oblique view to the CPU test's fp32
bound; eval_tsdf_depth's numbers equal independent NumPy ones; and an only-tracking run with tsdf.eval_depth ends with
metrics_tsdf_depth.txt."""
import math
import os
import random
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from go_slam_amd import synth                                  # noqa: E402
import test_tsdf_gpu as TG                                     # noqa: E402  (its lattice, frames and whole run)
import test_tsdf_raycast_cpu as RC                             # noqa: E402  (the plane scene and its bounds)
import tsdf_raycast_restatement as RR                          # noqa: E402
import tsdf_restatement as TR                                  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

H, W = TG.H, TG.W                                              # 48 x 64
INTR = (0.9 * W, 0.9 * W, 32.0, 24.0)                          # integer cx: column 32 has dx == 0 exactly
LO = [b[0] for b in TG.BOUND_EXACT]
KEYS = ("depth", "normal", "color")


def bits(t):
    t = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t
    return np.ascontiguousarray(t, dtype=np.float32).view(np.int32)


def assert_same(out, ref, keys=KEYS, frames=slice(None)):
    for k in keys:
        assert np.array_equal(bits(out[k]), bits(ref[k][frames])), k
    assert np.array_equal(out["depth"].cpu().numpy() > 0, ref["depth"][frames] > 0)


def w2c_of(c2w34):
    m = np.eye(4)
    m[:3] = c2w34
    return np.linalg.inv(m)


@pytest.fixture(scope="module")
def scene(built_lib):
    """The 37 x 21 x 70 lattice of test_tsdf_gpu.py fused on the GPU from its arc frames, six poses as world-to-camera
    matrices (three of the arc, one outside the box looking in, one with identity rotation, one looking away), the
    camera-to-world matrices the kernel is handed, and the restatement's images at three step lengths."""
    from go_slam_amd.lietorch_shim import SE3
    from go_slam_amd.tsdf import c2w_matrices
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
    arc = SE3(poses[[0, K // 2, K - 1]].double()).matrix().numpy()
    extra = [w2c_of(RC.look(90.0, 0.0, (-2.5, 0.3, 2.0))),             # outside the box (x < -1.5), looking along +x
             w2c_of(RC.cam((0.7, 0.4, -0.5))[0]),                      # identity rotation
             w2c_of(RC.cam((0.75, 0.5, -3.0), np.diag([-1.0, 1.0, -1.0]))[0])]   # behind the lattice, looking away
    w2c = torch.from_numpy(np.concatenate([arc, np.stack(extra)]))     # float64 [6,4,4]
    c2w = c2w_matrices(w2c).numpy()
    assert np.array_equal(c2w[4, :, :3], np.eye(3, dtype=np.float32))
    host = {"tsdf": vol.tsdf.cpu().numpy(), "weight": vol.weight.cpu().numpy(), "colors": vol.colors.cpu().numpy()}
    ref = {step: RR.raycast(host, c2w if step == 0.5 else c2w[[0, 3, 4]], INTR, (H, W), LO, TG.VOXEL, step=step)
           for step in (0.5, 1.0, 0.25)}
    return types.SimpleNamespace(vol=vol, w2c=w2c, c2w=c2w, host=host, ref=ref)


def test_images_equal_the_restatement_bit_for_bit(scene):
    """HIP's fp32 division and sqrtf are correctly rounded in this build (no fast-math flag), so the normals are held to
    the same standard as depth and colour."""
    ref = scene.ref[0.5]
    hit = ref["depth"] > 0
    print("hit share per pose:", hit.reshape(6, -1).mean(1))
    assert (hit[:5].reshape(5, -1).mean(1) > 0.1).all() and (~hit[:5]).any()
    assert hit[4][:, 32].any()                                 # the column with dx == 0 finds the wall
    assert len(np.unique(ref["color"][hit], axis=0)) > 100 and np.abs(ref["normal"][hit]).max() <= 1.0
    out = scene.vol.raycast(scene.w2c, INTR, (H, W))
    assert out["depth"].shape == (6, H, W) and out["normal"].shape == (6, H, W, 3) and out["color"].shape == (6, H, W, 3)
    assert out["depth"].dtype == torch.float32 and out["depth"].device == scene.vol.device
    assert_same(out, ref)


def test_brick_skip_changes_nothing_and_is_exercised(scene):
    flags = scene.vol.brick_flags().cpu().numpy()
    assert flags.shape == (5, 3, 9)                            # 70 points along z: nine bricks, the last one partial
    assert np.array_equal(flags, RR.brick_flags(scene.host["tsdf"]))
    print("flagged bricks:", int(flags.sum()), "of", flags.size)
    assert (flags == 0).any() and (flags != 0).any()
    stats = {}
    RR.raycast(scene.host, scene.c2w[:1], INTR, (H, W), LO, TG.VOXEL, flags=flags, stats=stats)
    assert stats["evaluated"] < stats["samples"]               # rays of these poses do cross unflagged bricks
    skipped = scene.vol.raycast(scene.w2c, INTR, (H, W), skip=True)
    plain = scene.vol.raycast(scene.w2c, INTR, (H, W), skip=False)
    assert_same(plain, scene.ref[0.5])
    assert_same(skipped, {k: plain[k].cpu().numpy() for k in KEYS})


def test_two_calls_and_a_split_call_give_the_same_bits(scene):
    a = scene.vol.raycast(scene.w2c, INTR, (H, W))
    b = scene.vol.raycast(scene.w2c, INTR, (H, W))
    first, rest = scene.vol.raycast(scene.w2c[:2], INTR, (H, W)), scene.vol.raycast(scene.w2c[2:], INTR, (H, W))
    for k in KEYS:
        assert np.array_equal(bits(a[k]), bits(b[k]))
        assert np.array_equal(bits(torch.cat([first[k], rest[k]])), bits(a[k]))
    empty = scene.vol.raycast(scene.w2c[:0], INTR, (H, W))
    assert empty["depth"].shape == (0, H, W)


@pytest.mark.parametrize("step", [1.0, 0.25])
def test_other_step_lengths_equal_their_own_restatement(scene, step):
    out = scene.vol.raycast(scene.w2c[[0, 3, 4]], INTR, (H, W), step=step)
    assert (scene.ref[step]["depth"] > 0).any()
    assert not np.array_equal(scene.ref[step]["depth"], scene.ref[0.5]["depth"][[0, 3, 4]])
    assert_same(out, scene.ref[step])


def test_without_colour_depth_and_normal_are_unchanged(scene):
    out = scene.vol.raycast(scene.w2c, INTR, (H, W), color=False)
    assert out["color"] is None
    assert_same(out, scene.ref[0.5], keys=("depth", "normal"))


def test_looking_away_and_unreachable_min_weight_give_zero_images(scene):
    assert not (scene.ref[0.5]["depth"][5] > 0).any()
    out = scene.vol.raycast(scene.w2c, INTR, (H, W))
    for k in KEYS:
        assert not bool(out[k][5].any())
    assert float(scene.vol.weight.max()) < 1000.0
    out = scene.vol.raycast(scene.w2c, INTR, (H, W), min_weight=1000.0)
    for k in KEYS:
        assert not bool(out[k].any())


def test_ragged_pixel_tiles(scene):
    """13 x 19 pixels: neither is a multiple of the 8 x 8 tile."""
    intr = (17.0, 17.0, 9.0, 6.0)
    ref = RR.raycast(scene.host, scene.c2w[[1, 4]], intr, (13, 19), LO, TG.VOXEL)
    assert (ref["depth"] > 0).any()
    out = scene.vol.raycast(scene.w2c[[1, 4]], intr, (13, 19))
    assert_same(out, ref)


def test_nan_pose_gives_a_zero_frame(scene):
    w2c = scene.w2c[[0, 1]].clone()
    w2c[0, 1, 3] = float("nan")
    out = scene.vol.raycast(w2c, INTR, (H, W))
    for k in KEYS:
        assert not bool(out[k][0].any())
        assert np.array_equal(bits(out[k][1]), bits(scene.ref[0.5][k][1]))


def test_oblique_plane_is_recovered_to_the_fp32_bound(built_lib):
    """test_tsdf_raycast_cpu.py's plane, fused and raycast on the GPU: the fp64 restatement is analytic to 1e-9 m there,
    fp32 within PLANE_FP32_BOUND of it, normals within PLANE_NORMAL_BOUND of (0, 0, -1)."""
    depth, w2c = TR.plane_scene(RC.PLANE_C)
    vol = TG.volume(TR.PLANE_BOUND, TR.PLANE_VOXEL)
    vol.integrate(torch.from_numpy(depth[:2]), torch.from_numpy(w2c[:2]), TR.PLANE_INTR)
    out = vol._raycast(torch.from_numpy(RC.PLANE_VIEW).float()[None], RC.INTR, RC.HW)      # the view, not its inverse's inverse
    d = out["depth"][0].cpu().numpy().astype(np.float64)
    truth = RC.plane_truth()
    hit = d > 0
    err = np.abs(d - truth)[hit].max()
    n_err = np.abs(out["normal"][0].cpu().numpy()[hit].astype(np.float64) - np.array([0.0, 0.0, -1.0])).max()
    print(f"{hit.sum()} hits, depth error {err:.3e} m (bound {RC.PLANE_FP32_BOUND:.3e}), normal error {n_err:.3e}")
    assert hit.mean() > 0.5
    assert err <= 1e-9 + RC.PLANE_FP32_BOUND
    assert n_err <= RC.PLANE_NORMAL_BOUND


def test_eval_tsdf_depth_against_numpy(built_lib, tmp_path):
    """synth.PlaneSequence's sensor depth fused at its poses (what fuse_keyframes(source="sensor") feeds the volume),
    then evaluated at those poses."""
    from go_slam_amd import tsdf
    seq = synth.PlaneSequence(16, 64, 96, 0.9 * 96, 0.9 * 96, 96 / 2 - 0.5, 64 / 2 - 0.5)
    w2c = torch.linalg.inv(seq.c2w.double())[:, :3, :].float()
    vol = TG.volume([[-4, 4], [-3, 2], [-1, 5]], 0.1)
    vol.integrate(seq.depths, w2c, seq.intrinsic.tolist(), images=seq.images)
    path = str(tmp_path / "metrics_tsdf_depth.txt")
    res = tsdf.eval_tsdf_depth(vol, seq, seq.c2w, seq.intrinsic.tolist(), every=5, out_path=path, save_images=True,
                               return_images=True)
    assert res["frames"] == [0, 5, 10, 15] and res["n_frames"] == 4
    pred = res["depth"].cpu().numpy()
    hit = res["hit"].cpu().numpy()
    assert np.array_equal(hit, pred > 0) and hit.any()
    rows = []
    for j, i in enumerate(res["frames"]):
        gt = seq.depths[i].numpy()
        valid = gt > 0
        both = valid & hit[j]
        l1 = np.abs(pred[j].astype(np.float64) - gt.astype(np.float64))[both].mean()
        rows.append((l1, both.sum() / valid.sum(), both.sum(), valid.sum()))
        assert res["per_frame"][j, 1] == rows[-1][1] and res["per_frame"][j, 2] == rows[-1][2]
        assert res["per_frame"][j, 3] == rows[-1][3]
        assert abs(res["per_frame"][j, 0] - l1) <= 1e-12 * l1
    print("per frame (depth_l1 m, coverage, n_depth, n_valid):", rows)
    assert res["coverage"] == sum(r[1] for r in rows) / 4 and res["coverage"] > 0.5
    assert abs(res["depth_l1_cm"] - 100 * sum(r[0] for r in rows) / 4) <= 1e-10
    assert res["depth_l1_cm"] < 10.0                           # one voxel: the scene, not a bound on the method
    back, lines = tsdf.parse_depth_metrics(open(path).read())
    assert back == {k: res[k] for k in tsdf.DEPTH_REPORT_ORDER}
    assert [(l[0], l[1], l[2], l[3]) for l in lines] == \
        [(i, float(r[0]), float(r[1]), int(r[2])) for i, r in zip(res["frames"], res["per_frame"])]
    assert sorted(os.listdir(tmp_path / "tsdf_eval")) == ["00000.jpg", "00005.jpg", "00010.jpg", "00015.jpg"]
    nan = tsdf.eval_tsdf_depth(vol, seq, seq.c2w, seq.intrinsic.tolist(), out_path=path, metric_depth=False)
    assert nan["n_frames"] == 0 and math.isnan(nan["depth_l1_cm"]) and "not rgbd" in open(path).read()


def whole_run(out_dir, tsdf_cfg):
    """test_tsdf_gpu.py's whole_run, keeping what terminate returns."""
    from go_slam_amd.slam import SLAM
    torch.manual_seed(43)
    torch.cuda.manual_seed_all(43)
    np.random.seed(43)
    random.seed(43)
    cfg = TG.make_cfg(out_dir, True)
    cfg["tsdf"] = tsdf_cfg
    slam = SLAM(types.SimpleNamespace(device="cuda:0", make_video=False, output=None), cfg, full_ba_every=4)
    with torch.no_grad():
        slam.net.update.delta[2].weight.mul_(0.02)
        slam.net.update.delta[2].bias.zero_()
    slam.ba.frontend_window = 8
    stream = synth.PlaneSequence(TG.N_RUN, TG.H_RUN, TG.W_RUN, 0.9 * TG.W_RUN, 0.9 * TG.W_RUN, TG.W_RUN / 2 - 0.5,
                                 TG.H_RUN / 2 - 0.5)
    slam.run(stream)
    stats = slam.terminate(rank=-1, stream=stream)
    torch.cuda.synchronize()
    return stats


def test_only_tracking_run_ends_with_metrics_tsdf_depth(built_lib, tmp_path):
    from go_slam_amd import tsdf
    with_dir, without_dir = str(tmp_path / "with"), str(tmp_path / "without")
    base = {"enable": True, "source": "sensor", "voxel_size": 0.1}
    stats = whole_run(with_dir, {**base, "eval_depth": {"enable": True, "every": 5}})
    plain = whole_run(without_dir, base)
    res, lines = tsdf.parse_depth_metrics(open(f"{with_dir}/metrics_tsdf_depth.txt").read())
    print("metrics_tsdf_depth.txt:", res, lines)
    assert [l[0] for l in lines] == [0, 5, 10, 15] and res["n_frames"] == 4
    assert {k: stats[f"tsdf_{k}"] for k in tsdf.DEPTH_REPORT_ORDER} == res
    assert res["coverage"] > 0 and math.isfinite(res["depth_l1_cm"])
    assert not os.path.exists(f"{without_dir}/metrics_tsdf_depth.txt")
    assert not any(k.startswith("tsdf_") for k in plain)
    assert sorted(plain) == sorted(k for k in stats if not k.startswith("tsdf_"))
    for k, v in plain.items():
        assert np.array_equal(np.asarray(v), np.asarray(stats[k])), k
    assert [p for p in TG.listing(with_dir) if p != "metrics_tsdf_depth.txt"] == TG.listing(without_dir)
