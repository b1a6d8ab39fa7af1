"""Stage times of one in-process run on one GPU (go_slam_amd.slam.SLAM), written to profiles/slam_run.json:
    python tools/slam_run_bench.py [--frames 48] [--size 240 320] [--out profiles/slam_run.json]
Sequence: synth.PlaneSequence (RGB-D, a wall and a floor from an arc), random DroidNet with small output heads and
motion_filter.thresh = 0, so every frame is a keyframe: the times say what the stages cost on that many keyframes, not
how well anything tracks.  Wall times per stage with a device synchronisation before and after each call:
  tracker / multiview_filter / mapper / ba during the stream (totals and call counts), the calls after the stream,
  and the pieces of terminate: checkpoint, trajectory filler, trajectory evaluation, mesher.
The trajectory evaluation is also timed on its own at the run's frame count and at 2000 frames: kernel launches (from
the library's kernel timer) and wall time of world_poses + ape on the device, beside the only route the package had
before: lietorch_shim composition on the device, a host copy, and eval_ate.ate_rmse in NumPy.  A record, no target."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from go_slam_amd import _lib, eval_ate, synth, traj_eval    # noqa: E402
from go_slam_amd.lietorch_shim import SE3                    # noqa: E402
from go_slam_amd.slam import SLAM                            # noqa: E402


def make_cfg(H, W, frames, out_dir):
    dev = "cuda:0"
    return {
        "sync_method": "strict", "verbose": False, "dataset": "synthetic", "mode": "rgbd", "stride": 1,
        "only_tracking": False,
        "mapping": {"device": dev, "BA": False, "BA_cam_lr": 0.001, "net_lr": 0.001, "grid_lr": 0.01,
                    "w_color_loss": 2.0, "w_sdf_smooth_loss": 1.0, "w_sdf_loss": 2.0, "w_eikonal_loss": 0.1,
                    "uncertainty_weight_loss": True, "mapping_window_size": 22, "pixels": 4400, "iters": 2,
                    "post_processing_iters": 10, "decay": 0.8, "bound": [[-4.0, 6.0], [-3.0, 2.0], [-1.0, 5.0]],
                    "model": {"sdf_smooth_std": 0.005, "sdf_sparse_factor": 5, "sdf_truncation": 0.16,
                              "sdf_random_weight": 0.04, "sdf_network": {"d_in": 3, "d_out": 32},
                              "color_network": {"d_in": 3, "d_feat": 31, "d_hidden": 64, "n_layers": 2},
                              "variance_network": {"init_val": 0.2, "scale_factor": 10.0}}},
        "tracking": {"device": dev, "pretrained": None, "buffer": frames + 24, "beta": 0.75, "warmup": 8,
                     "upsample": True, "motion_filter": {"thresh": 0.0},
                     "multiview_filter": {"thresh": 0.05, "visible_num": 2, "kernel_size": 1, "bound_enlarge_scale": 1.10},
                     "frontend": {"enable_loop": True, "keyframe_thresh": 0.0, "thresh": 1e4, "window": 25, "radius": 1,
                                  "nms": 1, "max_factors": 75},
                     "backend": {"thresh": 1e4, "radius": 1, "nms": 5, "loop_window": 25, "loop_thresh": 1e4,
                                 "loop_radius": 1, "loop_nms": 12}},
        "cam": {"H": H, "W": W, "fx": 0.9 * W, "fy": 0.9 * W, "cx": W / 2 - 0.5, "cy": H / 2 - 0.5,
                "png_depth_scale": 1000.0, "calibration_txt": "", "H_edge": 0, "W_edge": 0, "H_out": H, "W_out": W},
        "rendering": {"N_samples": 24, "N_surface": 48, "lindisp": False, "perturb": 1.0},
        "data": {"input_folder": "synthetic", "output": out_dir, "video_length": ""},
        "meshing": {"level_set": 0, "resolution": 128, "eval_rec": False, "get_largest_components": False,
                    "remove_small_geometry_threshold": 0.2, "n_points_to_eval": 200000, "mesh_threshold_to_eval": 0.05,
                    "gt_mesh_path": "", "forecast_radius": 0},
    }


class Stage:
    """wraps a worker: device-synchronised wall time of every call, split into `during` the stream and `after` it"""

    def __init__(self, inner, log, name):
        self.inner, self.log, self.name = inner, log, name

    def __getattr__(self, key):
        return getattr(self.inner, key)

    def __call__(self, *args, **kwargs):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = self.inner(*args, **kwargs)
        torch.cuda.synchronize()
        self.log.setdefault(self.name, []).append((time.perf_counter() - t) * 1e3)
        return out


def summary(ms):
    return {"calls": len(ms), "total_ms": round(sum(ms), 3), "median_ms": round(statistics.median(ms), 3),
            "max_ms": round(max(ms), 3)} if ms else {"calls": 0}


def wall(fn, reps=5):
    ts = []
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return round(statistics.median(ts[1:]), 4)


def evaluation_record(n, device):
    g = torch.Generator().manual_seed(n)
    w2c = synth.arc_poses(n).to(device)
    w2c[:, :3] += 0.01 * torch.randn(n, 3, generator=g).to(device)
    comp = torch.tensor([0, 0, 0, 0, 0, 0, 1.0], device=device)
    gt = SE3(synth.arc_poses(n).double()).inv().matrix()[:, :3, 3].contiguous().to(device)

    def native():
        tq, c2w = traj_eval.world_poses(w2c, comp)
        return traj_eval.ape(c2w[:, :3, 3].float().double().contiguous(), gt)

    def host_route():
        traj = SE3(comp[None]) * SE3(w2c).inv()
        est = traj.matrix().data.cpu().numpy()
        return eval_ate.ate_rmse(est[:, :3, 3].astype(np.float64), gt.cpu().numpy())
    a, (b, _) = native(), host_route()
    with _lib.kernel_timer(device) as timer:
        native()
        torch.cuda.synchronize()
    kernels = timer.read()
    return {"frames": n, "native_wall_ms": wall(native), "host_route_wall_ms": wall(host_route),
            "native_kernel_launches": int(sum(c for _, c in kernels.values())),
            "native_kernel_ms": round(sum(ms for ms, _ in kernels.values()), 4),
            "kernels": {k: [round(ms, 4), c] for k, (ms, c) in kernels.items()},
            "rmse_native": a["rmse"], "rmse_host_route": b}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--size", type=int, nargs=2, default=[240, 320])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "slam_run.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    H, W = a.size
    torch.manual_seed(43)
    np.random.seed(43)
    out_dir = tempfile.mkdtemp(prefix="slam_run_")
    cfg = make_cfg(H, W, a.frames, out_dir)
    args = types.SimpleNamespace(device="cuda:0", make_video=False, output=None)
    t0 = time.perf_counter()
    slam = SLAM(args, cfg)
    with torch.no_grad():
        slam.net.update.delta[2].weight.mul_(0.02)
        slam.net.update.delta[2].bias.zero_()
    torch.cuda.synchronize()
    construct_ms = (time.perf_counter() - t0) * 1e3
    log = {}
    for name in ("tracker", "ba", "multiview_filter", "mapper", "traj_filler", "mesher"):
        setattr(slam, name, Stage(getattr(slam, name), log, name))
    stream = synth.PlaneSequence(a.frames, H, W, 0.9 * W, 0.9 * W, W / 2 - 0.5, H / 2 - 0.5)
    t0 = time.perf_counter()
    slam.run(stream)
    torch.cuda.synchronize()
    run_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    stats = slam.terminate(rank=-1, stream=stream)
    torch.cuda.synchronize()
    terminate_ms = (time.perf_counter() - t0) * 1e3
    rec = {"device": torch.cuda.get_device_name(0), "frames": a.frames, "size": [H, W],
           "keyframes": int(slam.video.counter.value), "full_ba_every": slam.full_ba_every,
           "construct_ms": round(construct_ms, 1), "run_ms": round(run_ms, 1), "terminate_ms": round(terminate_ms, 1),
           "stages": {k: summary(v) for k, v in log.items()},
           "terminate_other_ms": round(terminate_ms - sum(log.get("traj_filler", [])) - sum(log.get("mesher", [])), 1),
           "ape": {k: stats[k] for k in traj_eval.STAT_NAMES},
           "outputs": sorted(os.path.relpath(os.path.join(d, f), out_dir) for d, _, fs in os.walk(out_dir) for f in fs),
           "trajectory_evaluation": [evaluation_record(n, "cuda:0") for n in (a.frames, 2000)],
           "note": "random DroidNet, every frame a keyframe; wall times with a device synchronisation around each call; "
                   "terminate_other_ms = checkpoint, trajectory evaluation, file writes"}
    txt = json.dumps(rec, indent=1)
    print(txt)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(txt + "\n")


if __name__ == "__main__":
    main()
