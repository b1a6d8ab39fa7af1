"""Frontier clusters on one GPU, written to profiles/frontier.json:
    timeout -k 10 900 python tools/frontier_bench.py [--reps 5] [--n 256] [--no-host] [--also LIB ...] [--out FILE]
The n^3 lattice over 8 m of tools/geodesic_bench.py -- a box room with a solid shell, split by a wall with one door (1 m
wide) -- with weight 0 at every x beyond the wall, so the far half was never observed; its distance field built with
max_distance 1 m.  With a robot of 0.25 m, medians of --reps runs of
  `frontier.frontier_clusters` on the field's state and passability alone: the kernels' own times (library kernel timer:
  frontier_mark, frontier_relax summed over its sweeps, and the table's frontier_count, frontier_scan, frontier_emit and
  frontier_table), the wall time of the call and the number of sweeps;
  the wall time of `ESDF.frontiers` and `ESDF.explore` from the start of tools/geodesic_bench.py, which add passability,
  snapping, the cost-to-go field (geodesic_* kernels, recorded too) and, for explore, the walk;
and, unless --no-host, the wall time of scipy.ndimage.label (26-connectivity) over the same frontier mask and of a numpy
table (bincount, ndimage.minimum, find_objects) on the host, and whether that partition and the roots equal the
kernels'.  The host code is one thread of another algorithm on another processor: the numbers are recorded, no ratio is
claimed.

--also: further builds of the library, each measured in a child process of its own (GOSLAM_HIP_LIB) and recorded under
"builds" by the library's file name.  Such a build is csrc/frontier.hip compiled with the Makefile's flags plus, for
example, -DFRONTIER_B0=8 -DFRONTIER_B1=8 -DFRONTIER_B2=16 for another brick, -DFRONTIER_ROUNDS_MAX=32 for another cap on
the rounds inside LDS, or -DFRONTIER_SHORTCUT=0 for neighbour relaxation without label[label[c]], linked with the other
objects of csrc/ into a shared library of another name."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from go_slam_amd import _lib, frontier                             # noqa: E402
from go_slam_amd.tsdf import TSDFVolume                            # noqa: E402
import geodesic_bench                                              # noqa: E402  (its room)

DEV = "cuda:0"
TABLE_KERNELS = ("frontier_count", "frontier_scan", "frontier_emit", "frontier_table")
KERNELS = ("frontier_mark", "frontier_relax") + TABLE_KERNELS + ("geodesic_fill", "geodesic_seed", "geodesic_relax",
                                                                 "geodesic_path")
RADIUS = 0.25


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


def record(ms, wall):
    rec = {"s_wall": statistics.median(wall), "s_wall_all": wall}
    for k in KERNELS:
        if any(v != 0.0 for v in ms[k]):
            rec[f"ms_{k}_kernel"], rec[f"ms_{k}_kernel_all"] = statistics.median(ms[k]), ms[k]
    rec["ms_table_kernels"] = sum(statistics.median(ms[k]) for k in TABLE_KERNELS)
    rec["ms_frontier_kernels"] = sum(statistics.median(ms[k]) for k in KERNELS if k.startswith("frontier"))
    return rec


def host_clusters(state, open_):
    """Seconds of the marking, of scipy's labelling and of the numpy table on the host, the label image and the roots."""
    from scipy import ndimage
    t0 = time.perf_counter()
    fr = (state == 1) & (open_ != 0) & ndimage.binary_dilation(state == 0, ndimage.generate_binary_structure(3, 1),
                                                               border_value=0)
    t_mark = time.perf_counter() - t0
    t0 = time.perf_counter()
    comp, K = ndimage.label(fr, structure=np.ones((3, 3, 3)))
    t_label = time.perf_counter() - t0
    t0 = time.perf_counter()
    ids = np.arange(1, K + 1)
    at = np.flatnonzero(fr)
    row = comp.ravel()[at] - 1
    roots = np.asarray(ndimage.minimum(np.arange(state.size, dtype=np.int64).reshape(state.shape), comp, ids)).reshape(K)
    size = np.bincount(row, minlength=K)
    coords = np.unravel_index(at, state.shape)
    sums = np.stack([np.bincount(row, weights=c, minlength=K) for c in coords], axis=1) if K else np.zeros((0, 3))
    boxes = ndimage.find_objects(comp)
    t_table = time.perf_counter() - t0
    return t_mark, t_label, t_table, comp, roots, size, sums, boxes


def measure(n, reps):
    voxel = 8.0 / n
    vol = TSDFVolume([[0.0, (n - 1) * voxel]] * 3, voxel, device=DEV)
    assert vol.dims == (n, n, n), vol.dims
    vol.tsdf.copy_(torch.from_numpy(geodesic_bench.room(n)))
    vol.weight.fill_(1.0)
    vol.weight[n // 2 + 1:] = 0.0                           # never observed beyond the wall
    field = vol.esdf(1.0)
    start = [c * voxel for c in (n // 8, n // 4, 7 * n // 8)]
    passable = field.passable(RADIUS)
    frontier.frontier_clusters(field.state, passable)       # warm-up
    field.explore(start, robot_radius=RADIUS)
    rec = {"brick": list(frontier.brick()), "lattice": [n, n, n], "voxel": voxel, "robot_radius": RADIUS,
           "sweep_batch": frontier.SWEEP_BATCH}
    c_ms, c_wall, c_res = timed(lambda: frontier.frontier_clusters(field.state, passable), reps)
    fc = c_res[-1]
    assert all(torch.equal(r.label, fc.label) and torch.equal(r.sum, fc.sum) for r in c_res)
    rec["clusters"] = {**record(c_ms, c_wall), "sweeps": [r.sweeps for r in c_res], "n_clusters": fc.n_clusters,
                       "counts": [int(v) for v in fc.counts.cpu().tolist()],
                       "largest_cluster_cells": int(fc.size.max().item()) if fc.n_clusters else 0}
    f_ms, f_wall, f_res = timed(lambda: field.frontiers(robot_radius=RADIUS, start=start), reps)
    rec["frontiers"] = {**record(f_ms, f_wall), "sweeps": [r.sweeps for r in f_res],
                        "field_sweeps": [r.field.sweeps for r in f_res],
                        "n_reachable": int((f_res[-1].best_cost < frontier.INF).sum().item())}
    e_ms, e_wall, e_res = timed(lambda: field.explore(start, robot_radius=RADIUS), reps)
    res = e_res[-1]
    assert res["reachable"] and all(torch.equal(r["cells"], res["cells"]) for r in e_res)
    rec["explore"] = {**record(e_ms, e_wall), "cluster": res["cluster"], "length_m": res["length_m"],
                      "min_clearance_m": res["min_clearance_m"], "path_cells": int(res["cells"].shape[0]),
                      "goal_cell": res["goal_cell"]}
    return rec, field, passable, fc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--also", nargs="*", default=[])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frontier.json"))
    a = ap.parse_args()
    rec, field, passable, fc = measure(a.n, a.reps)
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, **rec}
    print(json.dumps(out), flush=True)
    if not a.no_host:
        t_mark, t_label, t_table, comp, roots, size, sums, boxes = host_clusters(field.state.cpu().numpy(),
                                                                                 passable.cpu().numpy())
        label = fc.label.cpu().numpy()
        same = bool(np.array_equal(comp > 0, label >= 0)) and len(roots) == fc.n_clusters
        if same and len(roots):
            same = bool(np.array_equal(np.append(roots, -1)[comp - 1], label))       # comp 0 reads the -1
            order = np.argsort(roots)
            same = same and bool(np.array_equal(roots[order], fc.root.cpu().numpy()))
            same = same and bool(np.array_equal(size[order], fc.size.cpu().numpy()))
            same = same and bool(np.array_equal(sums[order].astype(np.int64), fc.sum.cpu().numpy()))
        out["host"] = {"s_scipy_mark_wall": t_mark, "s_scipy_label_wall": t_label, "s_numpy_table_wall": t_table,
                       "partition_and_table_equal_host": same}
        print(json.dumps(out["host"]), flush=True)
    if a.also:
        out["builds"] = {}
        for lib in a.also:
            tmp = os.path.abspath(a.out) + ".child"
            env = dict(os.environ, GOSLAM_HIP_LIB=os.path.abspath(lib))
            subprocess.run([sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--n", str(a.n), "--no-host",
                            "--out", tmp], env=env, check=True, timeout=300)
            with open(tmp) as fh:
                child = json.load(fh)
            os.remove(tmp)
            out["builds"][os.path.basename(lib)] = {k: child[k] for k in ("brick", "clusters", "frontiers", "explore")}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
