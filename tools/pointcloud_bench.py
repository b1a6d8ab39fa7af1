"""Keyframe point cloud on one GPU, written to profiles/pointcloud.json:
    python tools/pointcloud_bench.py [--reps 7] [--out profiles/pointcloud.json] [--no-launches]
Two paths over the same DepthVideo, run alternately (median wall time, the host's numpy arrays as the end state):
  (a) reference: animation_callback's data path (src/visualization.py:116-150) on this project's ops -- index_select,
      droid_backends.iproj over the dirty keyframes, depth_filter over the whole buffer, .cpu() of images, points,
      counts and disparities, the torch masks and per-keyframe boolean indexing on the host;
  (b) fused: go_slam_amd.pointcloud.keyframe_point_cloud, then PointCloud.numpy() (also timed without the host copy).
Per case: milliseconds, device launches and memory copies (torch.profiler, unless --no-launches), peak device memory
above what was allocated before the call, output points, and the count pass's time (library kernel timer) with the
bytes it must move at least: the listed keyframes' and their neighbour slots' disparities, the keep words and counts.
Scene: synth poses and the inverse depth of two planes (synth.plane_disps), random RGB."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from go_slam_amd import _lib, droid_backends as db, synth          # noqa: E402
from go_slam_amd.depth_video import DepthVideo                     # noqa: E402
from go_slam_amd.lietorch_shim import SE3                          # noqa: E402
from go_slam_amd import pointcloud as PC                           # noqa: E402

HBM_PEAK_GBS = 8000.0
DEV = "cuda:0"
CASES = [  # name, synth shape, buffer slots, counter, listed keyframes
    ("replica_200_of_250", "Rep", 250, 200, list(range(200))),
    ("s480_200_of_250", "S480", 250, 200, list(range(200))),
    ("replica_window_8", "Rep", 250, 200, list(range(150, 158))),
]


def make_video(shape, buffer, counter):
    h8, w8, _ = synth.SHAPES[shape]
    v = DepthVideo(h8, w8, buffer=buffer, device=DEV, full_res=True)
    syn = synth.make_video(buffer, shape, buffer=buffer)
    v.poses[:] = syn["poses"].to(DEV)
    v.intrinsics[:] = syn["intrinsics"].to(DEV)
    for a in range(0, buffer, 32):
        b = min(buffer, a + 32)
        v.disps_up[a:b] = synth.plane_disps(v.poses[a:b], v.intrinsics[0] * 8, v.ht, v.wd)
    v.images.copy_(torch.rand(v.images.shape, device=DEV))
    v.counter = counter
    return v


def reference(video, dirty_index, filter_thresh=0.01):
    """animation_callback's data path, camera actors aside"""
    images = torch.index_select(video.images, dim=0, index=dirty_index)
    images = images.cpu().permute(0, 2, 3, 1)
    intrinsic = video.intrinsics[0] * 8
    poses = torch.index_select(video.poses, dim=0, index=dirty_index)
    disps = torch.index_select(video.disps_up, dim=0, index=dirty_index)
    points = db.iproj(SE3(poses).inv().data.contiguous(), disps, intrinsic).cpu()
    thresh = filter_thresh * torch.ones_like(disps.mean(dim=[1, 2]))
    count = db.depth_filter(video.poses, video.disps_up, intrinsic, dirty_index, thresh)
    count = count.cpu()
    disps = disps.cpu()
    masks = ((count >= 2) & (disps > 0.01 * disps.mean(dim=[1, 2], keepdim=True)))
    out = []
    for i in range(len(dirty_index)):
        mask = masks[i].reshape(-1)
        out.append((points[i].reshape(-1, 3)[mask].numpy(), images[i].reshape(-1, 3)[mask].numpy()))
    return sum(len(p) for p, _ in out)


def fused(video, dirty_index, host=True):
    cloud = PC.keyframe_point_cloud(video, dirty_index)
    if host:
        cloud.numpy()
    return len(cloud)


def wall_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    n = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, n


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def launches(fn):
    from torch.profiler import profile, ProfilerActivity
    from torch.autograd import DeviceType
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    dev = [e for e in prof.events() if e.device_type == DeviceType.CUDA]
    copies = [e for e in dev if "memcpy" in e.name.lower() or "copy" in e.name.lower() and "Kernel" not in e.name]
    return {"kernels": len(dev) - len(copies), "copies": len(copies)}


def count_pass_bytes(listed, num, hw, k):
    """disparities of the listed keyframes and of every neighbour slot they read, keep words, survivor counts"""
    slots = set()
    for ix in listed:
        slots.add(ix)
        slots.update(j for j in (ix - 1, ix - 2, ix - 3, ix + 3, ix + 4, ix + 5) if 0 <= j < num)
    tiles = (hw + 1023) // 1024
    return len(slots) * hw * 4 + k * tiles * (16 * 8 + 4)


def run_case(name, shape, buffer, counter, listed, reps, with_launches):
    video = make_video(shape, buffer, counter)
    idx = torch.tensor(listed, device=DEV)
    hw = video.ht * video.wd
    ref = lambda: reference(video, idx)            # noqa: E731
    fus = lambda: fused(video, idx)                # noqa: E731
    dev_only = lambda: fused(video, idx, host=False)   # noqa: E731
    n_ref, n_fus = ref(), fus()                    # warm-up
    dev_only()
    ta, tb, tc = [], [], []
    for _ in range(reps):                          # alternating
        ta.append(wall_ms(ref)[0])
        tb.append(wall_ms(fus)[0])
        tc.append(wall_ms(dev_only)[0])
    with _lib.kernel_timer(DEV) as kt:
        dev_only()
        torch.cuda.synchronize()
    kstats = kt.read()
    count_ms = kstats.get("pointcloud_count", (float("nan"), 0))[0]
    nbytes = count_pass_bytes(listed, buffer, hw, len(listed))
    res = {
        "shape": [video.ht, video.wd], "buffer": buffer, "counter": counter, "listed": len(listed),
        "points_reference": n_ref, "points_fused": n_fus,
        "ms_reference": statistics.median(ta), "ms_fused_to_host": statistics.median(tb),
        "ms_fused_on_device": statistics.median(tc),
        "ms_reference_all": ta, "ms_fused_to_host_all": tb,
        "peak_bytes_reference": peak_bytes(ref), "peak_bytes_fused": peak_bytes(fus),
        "library_kernels_fused": {k: {"ms": v[0], "launches": v[1]} for k, v in kstats.items()},
        "count_pass_ms": count_ms, "count_pass_min_bytes": nbytes,
        "count_pass_gbs": nbytes / (count_ms * 1e-3) / 1e9,
    }
    res["count_pass_fraction_of_hbm_peak"] = res["count_pass_gbs"] / HBM_PEAK_GBS
    if with_launches:
        try:
            res["launches_reference"] = launches(ref)
            res["launches_fused_to_host"] = launches(fus)
        except Exception as exc:      # noqa: BLE001 -- the profiler is optional; the timings stand without it
            res["launches_error"] = repr(exc)[:300]
    print(name, json.dumps({k: v for k, v in res.items() if not k.endswith("_all")}), flush=True)
    del video
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pointcloud.json"))
    ap.add_argument("--no-launches", action="store_true")
    a = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "cases": {}}
    for name, shape, buffer, counter, listed in CASES:
        out["cases"][name] = run_case(name, shape, buffer, counter, listed, a.reps, not a.no_launches)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
