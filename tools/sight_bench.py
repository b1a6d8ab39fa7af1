"""Line of sight and the straightened path on one GPU, written to profiles/sight.json:
    timeout -k 10 900 python tools/sight_bench.py [--reps 5] [--n 256] [--no-host] [--out FILE]
Two scenes on an n^3 lattice over 8 m, written straight into a TSDFVolume, distance field built with max_distance 1 m:
  "door"  tools/geodesic_bench.py's room split by a wall with one door, robot 0.25 m: a route with one bend;
  "maze"  the same shell with a wall every n/16 cells whose doors alternate between the two ends of the last axis, robot
          0.125 m: a route of a few thousand cells.
Per scene, medians of --reps runs of
  the kernels' own times per stage (library kernel timer: path_sight, path_shortcut, segment_min) inside
  `ESDF.plan(straighten=True)`, the wall time of that call beside the same call without the keyword in the same run, the
  number of cells and of waypoints and both lengths, and the share of the sequential programme in the three stages;
  a window table: for windows 64, 256, 1024 and L - 1 (cut to the path) the two kernels' times, the wall time of
  `plan.straighten` on the finished route, the number of waypoints and the straightened length;
and, unless --no-host, the wall time of the serial restatement (tests/sight_restatement.py) on the same path with the
default window and whether it keeps the same cells.  The restatement is interpreted Python on one host thread: the number
is recorded as the only comparator there is, no ratio is claimed."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from go_slam_amd import _lib, plan                                 # noqa: E402
from go_slam_amd.tsdf import TSDFVolume                            # noqa: E402
from geodesic_bench import room                                    # noqa: E402  (tools/: beside this file)

DEV = "cuda:0"
KERNELS = ("path_sight", "path_shortcut", "segment_min")
WINDOWS = (64, 256, 1024, None)                              # None: L - 1


def maze(n):
    """tsdf float32 [n,n,n]: the solid shell and a two-cell wall across axis 0 every n/16 cells, each with a door over the
    whole of axis 1 and 3n/32 cells of axis 2, at alternating ends."""
    t = np.ones((n, n, n), dtype=np.float32)
    t[0], t[-1], t[:, 0], t[:, -1], t[:, :, 0], t[:, :, -1] = -1, -1, -1, -1, -1, -1
    for k, x in enumerate(range(n // 16, n - 2, n // 16)):
        t[x:x + 2] = -1
        z0 = n // 32 if k % 2 == 0 else n - n // 32 - 3 * n // 32
        t[x:x + 2, 1:n - 1, z0:z0 + 3 * n // 32] = 1
    return t


def timed(fn, reps):
    """({kernel: [ms]}, [wall s], [results]) of fn over reps runs."""
    ms, wall, results = {k: [] for k in KERNELS}, [], []
    for _ in range(reps):
        torch.cuda.synchronize()
        with _lib.kernel_timer(DEV) as kt:
            t0 = time.perf_counter()
            results.append(fn())
            torch.cuda.synchronize()
            wall.append(time.perf_counter() - t0)
        got = kt.read()
        for k in KERNELS:
            ms[k].append(got.get(k, (0.0, 0))[0])
    return ms, wall, results


def measure(name, tsdf, n, radius, start, goal, reps, host):
    voxel = 8.0 / n
    vol = TSDFVolume([[0.0, (n - 1) * voxel]] * 3, voxel, device=DEV)
    assert vol.dims == (n, n, n), vol.dims
    vol.tsdf.copy_(torch.from_numpy(tsdf))
    vol.weight.fill_(1.0)
    field = vol.esdf(1.0)
    start, goal = [c * voxel for c in start], [c * voxel for c in goal]
    field.plan(start, goal, robot_radius=radius, straighten=True)            # warm-up
    s_ms, s_wall, s_res = timed(lambda: field.plan(start, goal, robot_radius=radius, straighten=True), reps)
    _, p_wall, p_res = timed(lambda: field.plan(start, goal, robot_radius=radius), reps)
    res = s_res[-1]
    assert res["reachable"] and all(torch.equal(r["waypoint_index"], res["waypoint_index"]) for r in s_res)
    assert torch.equal(p_res[-1]["cells"], res["cells"])
    L = int(res["cells"].shape[0])
    med = {k: statistics.median(s_ms[k]) for k in KERNELS}
    rec = {"lattice": [n, n, n], "voxel": voxel, "robot_radius": radius, "path_cells": L,
           "waypoints": int(res["waypoints"].shape[0]), "length_m": res["length_m"],
           "straight_length_m": res["straight_length_m"], "min_clearance_m": res["min_clearance_m"],
           "straight_min_clearance_m": res["straight_min_clearance_m"], "window": plan.DEFAULT_WINDOW,
           "s_wall_plan_straighten": statistics.median(s_wall), "s_wall_plan": statistics.median(p_wall),
           "s_wall_plan_straighten_all": s_wall, "s_wall_plan_all": p_wall,
           "ms_kernels": sum(med.values()), "share_path_shortcut": med["path_shortcut"] / sum(med.values())}
    for k in KERNELS:
        rec[f"ms_{k}_kernel"], rec[f"ms_{k}_kernel_all"] = med[k], s_ms[k]
    passable = field.passable(radius)
    rec["windows"] = []
    for window in WINDOWS:
        w = max(L - 1, 1) if window is None else window
        plan.straighten(passable, res["cells"], w)                           # warm-up
        w_ms, w_wall, w_res = timed(lambda: plan.straighten(passable, res["cells"], w), reps)
        rec["windows"].append({"window": w_res[-1]["window"], "asked": "L-1" if window is None else window,
                               "ms_path_sight_kernel": statistics.median(w_ms["path_sight"]),
                               "ms_path_shortcut_kernel": statistics.median(w_ms["path_shortcut"]),
                               "s_wall_straighten": statistics.median(w_wall),
                               "waypoints": int(w_res[-1]["index"].shape[0]), "length": w_res[-1]["length"],
                               "length_m": w_res[-1]["length"] * voxel / 1000.0})
    print(json.dumps({name: rec}), flush=True)
    if host:
        import sight_restatement as SR
        p = passable.cpu().numpy() != 0
        cells = res["cells"].cpu().numpy()
        t0 = time.perf_counter()
        index, length = SR.straighten(p, cells, plan.DEFAULT_WINDOW)
        rec["host"] = {"s_restatement_wall": time.perf_counter() - t0, "window": plan.DEFAULT_WINDOW,
                       "equals_restatement": bool(np.array_equal(index, res["waypoint_index"].cpu().numpy())
                                                  and length * voxel / 1000.0 == res["straight_length_m"])}
        print(json.dumps({name: rec["host"]}), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sight.json"))
    a = ap.parse_args()
    n = a.n
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps}
    out["door"] = measure("door", room(n), n, 0.25, (n // 8, n // 4, 7 * n // 8), (7 * n // 8, n // 2, n // 8), a.reps,
                          not a.no_host)
    out["maze"] = measure("maze", maze(n), n, 0.125, (n // 32, n // 4, n // 2), (n - n // 32, n // 2, n // 2), a.reps,
                          not a.no_host)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
