"""Two whole runs of go_slam_amd.slam.SLAM on the GPU -- tracker, bundle adjustment, multiview filter, mapper, trajectory
filler, trajectory evaluation and mesher in one process -- on an in-memory sequence (synth.PlaneSequence: 16 RGB-D
frames at 64 x 96), and the files `terminate` writes.

The DroidNet is random (tracking.pretrained: None), so nothing here is about tracking accuracy: the tests check that the
workers run against one set of buffers in the documented order and that the outputs are what the reference's formats
say.  Every frame becomes a keyframe (motion_filter.thresh = 0)."""
import os
import types

import numpy as np
import pytest
import torch

import traj_eval_restatement as TR
from go_slam_amd import eval_ate

pytestmark = pytest.mark.gpu

N, H, W = 16, 64, 96
U32 = 2.0 ** -24


def make_cfg(out_dir, only_tracking):
    dev = "cuda:0"
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
        "cam": {"H": H, "W": W, "fx": 0.9 * W, "fy": 0.9 * W, "cx": W / 2 - 0.5, "cy": H / 2 - 0.5,
                "png_depth_scale": 1000.0, "calibration_txt": "", "H_edge": 0, "W_edge": 0, "H_out": H, "W_out": W},
        "rendering": {"N_samples": 24, "N_surface": 48, "lindisp": False, "perturb": 1.0},
        "data": {"input_folder": "synthetic", "output": out_dir, "video_length": ""},
        "meshing": {"level_set": 0, "resolution": 32, "eval_rec": False, "get_largest_components": False,
                    "remove_small_geometry_threshold": 0.2, "n_points_to_eval": 200000, "mesh_threshold_to_eval": 0.05,
                    "gt_mesh_path": "", "forecast_radius": 0},
    }


def make_stream(poses=True, timestamps=False):
    from go_slam_amd import synth
    return synth.PlaneSequence(N, H, W, 0.9 * W, 0.9 * W, W / 2 - 0.5, H / 2 - 0.5, poses=poses, timestamps=timestamps)


class MesherRecorder:
    def __init__(self, inner):
        self.inner, self.calls = inner, []

    def __call__(self, *args, **kwargs):
        self.calls.append((args, kwargs))
        return self.inner(*args, **kwargs)


def whole_run(out_dir, only_tracking):
    from go_slam_amd.slam import SLAM
    import random
    torch.manual_seed(43)
    torch.cuda.manual_seed_all(43)
    np.random.seed(43)
    random.seed(43)
    cfg = make_cfg(out_dir, only_tracking)
    args = types.SimpleNamespace(device="cuda:0", make_video=False, output=None)
    slam = SLAM(args, cfg, full_ba_every=4)
    with torch.no_grad():       # small output heads: a random network must not throw the poses to infinity
        slam.net.update.delta[2].weight.mul_(0.02)
        slam.net.update.delta[2].bias.zero_()
    slam.ba.frontend_window = 8                         # (25 keyframes would be needed otherwise: the BA has to run)
    slam.mesher = MesherRecorder(slam.mesher)
    stream = make_stream()
    slam.run(stream)
    stats = slam.terminate(rank=-1, stream=stream)
    torch.cuda.synchronize()
    return types.SimpleNamespace(slam=slam, stats=stats, out=out_dir, stream=stream)


@pytest.fixture(scope="module")
def tracking_run(built_lib, tmp_path_factory):
    return whole_run(str(tmp_path_factory.mktemp("only_tracking")), True)


@pytest.fixture(scope="module")
def mapping_run(built_lib, tmp_path_factory):
    return whole_run(str(tmp_path_factory.mktemp("with_mapping")), False)


def parse_metrics(path):
    lines = open(path).read().splitlines()
    assert lines[0].startswith("APE") and "translation" in lines[0] and "Umeyama" in lines[1] and "Sim(3)" in lines[1]
    rows = [l.split("\t") for l in lines[2:]]
    assert [r[0] for r in rows] == ["max", "mean", "median", "min", "rmse", "sse", "std"]
    return {k: float(v) for k, v in rows}


def check_outputs(run, frames=N, gt=None):
    from go_slam_amd.neus import InstantNeuS
    ckpt = torch.load(f"{run.out}/checkpoints/go.ckpt", map_location="cpu")
    assert sorted(ckpt) == ["keyframe_timestamps", "mapping_net", "tracking_net"]
    want = InstantNeuS(run.slam.cfg["mapping"]["model"], bound=run.slam.cfg["mapping"]["bound"], device="cuda:0").state_dict()
    assert list(ckpt["mapping_net"]) == list(want)
    assert list(ckpt["tracking_net"]) == list(run.slam.net.state_dict())
    assert ckpt["keyframe_timestamps"].shape[0] == 32
    poses = np.load(f"{run.out}/checkpoints/est_poses.npy")
    assert poses.dtype == np.float32 and poses.shape == (N, 4, 4) and np.isfinite(poses).all()
    assert (poses[:, 3] == np.array([0, 0, 0, 1], dtype=np.float32)).all()
    # Orthonormality, from the fp32 operation count.  A pose's quaternion is only ever multiplied by unit-norm updates
    # (gs_retr_se3: exp, then a quaternion product) and is never renormalised: each retraction moves |q|^2 by at most
    # 2 (7 + 6) u32 (7 rounded operations per component of the product, 6 in the exponential's sin / cos / scaling).  A
    # pose takes at most K = 130 retractions in these runs (frontend: at most 6 updates for each of 16 keyframes plus the
    # 16 of the initialisation; 2 full BAs of 6 steps; the filler's 6).  R(q) R(q)^T - I is 2 eps + eps^2 for
    # |q|^2 = 1 + eps, entries at most 4 eps with the off-diagonal terms; the fp32 store of R adds 2 u32 per product term.
    K = 130
    tol = 4 * K * 2 * (7 + 6) * U32 + 3 * 2 * U32
    R = poses[:, :3, :3].astype(np.float64)
    dev = np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max()
    print(f"orthonormality: {dev:.3e} (bound {tol:.3e})")
    assert dev <= tol
    if gt is None:
        return poses, None
    # metrics_traj.txt against eval_ate on the file's own positions and the GT, to the restatement's end-to-end bound
    stats = parse_metrics(f"{run.out}/metrics_traj.txt")
    valid = np.array([np.isfinite(p.sum()) for p in gt])
    est_xyz = poses[valid, :3, 3].astype(np.float64)
    ref_xyz = np.stack(gt)[valid, :3, 3].astype(np.float64)
    assert valid.sum() == frames
    rmse, info = eval_ate.ate_rmse(est_xyz, ref_xyz)
    err = np.linalg.norm(ref_xyz - (info["scale"] * (info["rotation"] @ est_xyz.T).T + info["translation"]), axis=1)
    want = {"rmse": rmse, "mean": info["mean"], "median": info["median"], "max": info["max"], "min": err.min(),
            "sse": (err ** 2).sum(), "std": err.std()}
    bound = TR.ape(est_xyz, ref_xyz)["bound"]
    for k, v in want.items():
        print(f"{k}: file {stats[k]!r} eval_ate {v!r} bound {bound[k]:.3e}")
        assert abs(stats[k] - v) <= 2 * bound[k], k
        assert stats[k] == run.stats[k]
    assert np.allclose(run.stats["alignment_transformation_sim3"], info["alignment_transformation_sim3"], atol=1e-6)
    return poses, stats


def test_only_tracking_run(tracking_run):
    run = tracking_run
    check_outputs(run, gt=run.stream.poses)
    assert run.stats["count"] == N
    assert run.slam.mesher.calls == []                   # nothing but the tracker and the BA
    assert not os.path.exists(f"{run.out}/mesh/final_raw_mesh.ply") and not os.path.exists(f"{run.out}/submission.txt")
    assert int(run.slam.video.counter.value) == N and int(run.slam.ba.last_t) == N
    assert int(run.slam.video.filtered_id.item()) <= 0 and run.slam.mapper.global_step == 0
    for flag in ("tracking_finished", "optimizing_finished", "mapping_finished", "meshing_finished"):
        assert int(getattr(run.slam, flag)) == 1


def test_run_with_mapping(mapping_run):
    run = mapping_run
    poses, _ = check_outputs(run, gt=run.stream.poses)
    assert run.slam.mapper.global_step > 0 and int(run.slam.video.filtered_id.item()) > 1
    assert os.path.exists(f"{run.out}/mesh/final_raw_mesh.ply")
    assert os.path.exists(f"{run.out}/cfg.yaml") is False            # run.py's file, not SLAM's
    # the alignment of the trajectory evaluation reaches the mesher, with the poses of the file
    (args, kwargs), = run.slam.mesher.calls
    assert args == () and kwargs["the_end"] is True
    assert kwargs["trans_init"] is run.stats["alignment_transformation_sim3"] and kwargs["trans_init"].shape == (4, 4)
    assert torch.equal(kwargs["estimate_c2w_list"], torch.from_numpy(poses))
    assert kwargs["gt_c2w_list"].shape == (N, 4, 4)


def test_stream_without_gt_writes_a_submission(tracking_run, tmp_path):
    run = tracking_run
    saved = run.slam.output
    try:
        run.slam.output = str(tmp_path)
        stats = run.slam.terminate(rank=-1, stream=make_stream(poses=False, timestamps=True))
    finally:
        run.slam.output = saved
    assert stats == {} and not os.path.exists(tmp_path / "metrics_traj.txt")
    lines = open(tmp_path / "submission.txt").read().splitlines()
    assert len(lines) == N
    poses = np.load(tmp_path / "checkpoints" / "est_poses.npy")
    for i, line in enumerate(lines):
        fields = line.split(" ")
        assert len(fields) == 8 and len(fields[0].split(".")[1]) == 9 and all(len(f.split(".")[1]) == 14 for f in fields[1:])
        assert float(fields[0]) == pytest.approx(0.1 * i, abs=1e-9)
        # half a unit of the 14th decimal, and the decimal string's own rounding to a double
        assert np.abs(np.array(fields[1:4], dtype=np.float64) - poses[i, :3, 3]).max() < 1e-14
    assert run.slam.mesher.calls == []


def test_nan_gt_pose_is_skipped(tracking_run, tmp_path, capsys):
    run = tracking_run
    stream = make_stream()
    stream.poses[5] = np.full((4, 4), np.nan, dtype=np.float32)
    saved = run.slam.output
    try:
        run.slam.output = str(tmp_path)
        capsys.readouterr()
        stats = run.slam.terminate(rank=-1, stream=stream)
        printed = capsys.readouterr().out
    finally:
        run.slam.output = saved
    assert [l for l in printed.splitlines() if "skipping" in l] == ["Nan or Inf found in gt poses, skipping 5th pose!"]
    assert stats["count"] == N - 1
    run2 = types.SimpleNamespace(slam=run.slam, stats=stats, out=str(tmp_path))
    check_outputs(run2, frames=N - 1, gt=stream.poses)
