"""Keeping a TSDF volume consistent during a run, on one GPU, written to profiles/tsdf_live.json:
    timeout -k 10 900 python tools/tsdf_live_bench.py [--reps 5] [--n 256] [--keyframes 64] [--out profiles/tsdf_live.json]
An n^3 lattice over 8 m and a video of K keyframes at 480 x 640 on synth's arc over its wall and floor.  Per source
("sensor", "tracked") and number B of moved keyframes:
  (a) live: B poses are moved by 10 cm and one LiveFusion.update() with budget B scores all K records and re-fuses the B
      (taken out at the old pose and added at the new one in one mixed-sign batch);
  (b) the only alternative without this feature: tsdf.fuse_keyframes over all K keyframes into a new volume.
Medians over the repetitions of the summed kernel times (the library's kernel timer, per launch name) and of the wall
time of the call; fuse_keyframes also extracts the mesh, so its marching-cubes launches are listed apart and left out of
`ms_kernels_fusion`, and the live side's resolve and mesh are timed apart as well.  The numbers are recorded; the file
gates nothing."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from go_slam_amd import _lib, synth                                # noqa: E402
from go_slam_amd.depth_video import DepthVideo                     # noqa: E402
from go_slam_amd.tsdf import fuse_keyframes                        # noqa: E402
from go_slam_amd.tsdf_live import LiveFusion                       # noqa: E402

DEV = "cuda:0"
FUSION_KERNELS = ("tsdf_integrate", "tsdf_accumulate", "tsdf_frame_change", "depth_filter")


def make_video(k):
    h8, w8, _ = synth.SHAPES["S480"]
    v = DepthVideo(h8, w8, buffer=k, device=DEV, full_res=True)
    v.poses[:] = synth.arc_poses(k).to(DEV)
    v.intrinsics[:] = torch.tensor([577.590698, 578.729797, 318.905426, 242.683609], device=DEV) / 8
    v.disps_up[:] = synth.plane_disps(v.poses, v.intrinsics[0] * 8, v.ht, v.wd)
    v.depths_gt[:] = torch.where(v.disps_up > 0, 1.0 / v.disps_up, torch.zeros_like(v.disps_up))
    v.images.copy_(torch.rand(v.images.shape, generator=torch.Generator(device=DEV).manual_seed(1), device=DEV))
    v.timestamp[:] = torch.arange(k, device=DEV)
    v.counter = k
    return v


def timed(fn):
    """(wall ms, {launch name: ms}, result) of fn."""
    torch.cuda.synchronize()
    with _lib.kernel_timer(DEV) as kt:
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t) * 1e3
    return wall, {name: ms for name, (ms, _) in kt.read().items()}, out


def summarise(runs):
    names = sorted({n for _, k, _ in runs for n in k})
    per = {n: statistics.median(k.get(n, 0.0) for _, k, _ in runs) for n in names}
    fusion = [sum(ms for n, ms in k.items() if n in FUSION_KERNELS) for _, k, _ in runs]
    return {"ms_wall": statistics.median(w for w, _, _ in runs), "ms_wall_all": [w for w, _, _ in runs],
            "ms_kernels_fusion": statistics.median(fusion), "ms_kernels_all_library": statistics.median(
                sum(k.values()) for _, k, _ in runs), "ms_per_kernel": per}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--keyframes", type=int, default=64)
    ap.add_argument("--moved", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsdf_live.json"))
    a = ap.parse_args()
    n, K = a.n, a.keyframes
    voxel, lo = 8.0 / n, (-4.0, -4.0, -2.0)
    bound = [[l, l + (n - 1) * voxel] for l in lo]
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "lattice": [n, n, n], "voxel": voxel, "keyframes": K,
           "image": [480, 640], "fusion_kernels": list(FUSION_KERNELS),
           "note": "ms_kernels_fusion sums the launches named in fusion_kernels; medians over reps", "cases": {}}
    for source in ("sensor", "tracked"):
        v = make_video(K)
        live = LiveFusion(v, bound, voxel, source=source, budget=max(a.moved), lag=0)
        assert live.volume_state.dims == (n, n, n)
        w, k, first = timed(live.update)
        assert first["integrated"] == K
        case = {"first_update_all_keyframes": {"ms_wall": w, "ms_per_kernel": k}}
        timed(lambda: fuse_keyframes(v, bound, voxel, source=source))                      # warm-up
        case["fuse_keyframes_all"] = summarise([timed(lambda: fuse_keyframes(v, bound, voxel, source=source))
                                                for _ in range(a.reps)])
        for B in a.moved:
            live.budget = B
            ids = torch.linspace(0, K - 1, B).round().long().unique().to(DEV)
            runs = []
            for r in range(a.reps + 1):
                v.poses[ids, :3] += 0.1 if r % 2 == 0 else -0.1
                run = timed(live.update)
                assert run[2]["refused"] == ids.numel() and run[2]["pending"] == 0, run[2]
                runs.append(run)
            case[f"update_moved_{B}"] = summarise(runs[1:])                              # the first one warms up
        runs = [timed(live.update) for _ in range(a.reps)]
        assert all(r[2]["refused"] == 0 for r in runs)
        case["update_nothing_moved"] = summarise(runs)
        live.volume_state._stale = True
        case["resolve"] = summarise([timed(lambda: (setattr(live.volume_state, "_stale", True), live.volume())[1])
                                     for _ in range(a.reps)])
        case["mesh_of_resolved"] = summarise([timed(live.mesh) for _ in range(3)])
        out["cases"][source] = case
        print(source, json.dumps({name: {"ms_wall": c["ms_wall"], "ms_kernels_fusion": c.get("ms_kernels_fusion")}
                                  for name, c in case.items()}), flush=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
        del live, v
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
