"""Cost-to-go field and paths on one GPU, written to profiles/geodesic.json:
    timeout -k 10 900 python tools/geodesic_bench.py [--reps 5] [--n 256] [--no-host] [--also LIB ...] [--out FILE]
An n^3 lattice over 8 m: a box room with a solid shell, split by a wall with one door (1 m wide), written straight into
a TSDFVolume, its distance field built with max_distance 1 m.  For `ESDF.plan` from one half to the far corner of the
other and for `ESDF.reachable` from the start, with a robot of 0.25 m, medians of --reps runs of
  the kernels' own times (library kernel timer: geodesic_fill, geodesic_seed, geodesic_relax summed over its sweeps,
  geodesic_path), the wall time of the whole call (passability, snapping, sweeps in batches with their reads, the walk)
  and the number of sweeps;
and, unless --no-host, the wall time of scipy.sparse.csgraph.dijkstra over the same allowed-move graph on the host (the
graph's construction is timed apart), and whether its distances equal the kernels' field.  The host search is one
thread of another algorithm on another processor: the numbers are recorded, no ratio is claimed.

--also: further builds of the library with another brick, each measured in a child process of its own (GOSLAM_HIP_LIB)
and recorded under "bricks" by the library's file name.  Such a build is csrc/geodesic.hip compiled with the
Makefile's flags plus, for example, -DGEO_B0=8 -DGEO_B1=8 -DGEO_B2=16 (and -DGEO_ROUNDS_MAX=32 for another cap on the
rounds inside LDS), linked with the other objects of csrc/ into a shared library of another name."""
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
from go_slam_amd import _lib, plan                                 # noqa: E402
from go_slam_amd.tsdf import TSDFVolume                            # noqa: E402

DEV = "cuda:0"
KERNELS = ("geodesic_fill", "geodesic_seed", "geodesic_relax", "geodesic_path")
RADIUS = 0.25


def room(n):
    """tsdf float32 [n,n,n]: -1 in the shell and in the wall at x = n/2 - 1, n/2 (door: y in [1, 3n/4), z in
    [7n/16, 9n/16)), +1 elsewhere."""
    t = np.ones((n, n, n), dtype=np.float32)
    t[0], t[-1], t[:, 0], t[:, -1], t[:, :, 0], t[:, :, -1] = -1, -1, -1, -1, -1, -1
    t[n // 2 - 1:n // 2 + 1] = -1
    t[n // 2 - 1:n // 2 + 1, 1:3 * n // 4, 7 * n // 16:9 * n // 16] = 1
    return t


def timed(fn, reps):
    """({kernel: median ms}, median wall s, [results]) of fn over reps runs."""
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


def host_dijkstra(passable, seed):
    """(seconds to build the graph, seconds of scipy's dijkstra, int64 distances [n0,n1,n2] with INF) on the host."""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import dijkstra
    n0, n1, n2 = passable.shape
    t0 = time.perf_counter()
    pad = np.zeros((n0 + 2, n1 + 2, n2 + 2), dtype=bool)
    pad[1:-1, 1:-1, 1:-1] = passable
    moves = [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if (a, b, c) != (0, 0, 0)]
    weight = np.array([{1: 1000, 2: 1414, 3: 1732}[sum(v != 0 for v in d)] for d in moves], dtype=np.float64)
    offset = np.array([(d[0] * n1 + d[1]) * n2 + d[2] for d in moves], dtype=np.int64)
    counts, cols, vals = [], [], []
    slab = max(1, (1 << 21) // (n1 * n2))                   # layers of axis 0 at a time: the masks stay small
    for a0 in range(0, n0, slab):
        a1 = min(a0 + slab, n0)
        ok = np.ones((a1 - a0, n1, n2, 26), dtype=bool)
        for m, d in enumerate(moves):
            for a in {0, d[0]}:
                for b in {0, d[1]}:
                    for c in {0, d[2]}:
                        ok[..., m] &= pad[1 + a0 + a:1 + a1 + a, 1 + b:1 + b + n1, 1 + c:1 + c + n2]
        ok = ok.reshape(-1, 26)
        cell, move = np.nonzero(ok)                         # by cell, then by move: CSR order
        counts.append(ok.sum(axis=1))
        cols.append((cell + a0 * n1 * n2 + offset[move]).astype(np.int32))
        vals.append(weight[move])
    indptr = np.concatenate([[0], np.cumsum(np.concatenate(counts))])
    graph = csr_matrix((np.concatenate(vals), np.concatenate(cols), indptr), shape=(passable.size, passable.size))
    t_graph = time.perf_counter() - t0
    t0 = time.perf_counter()
    d = dijkstra(graph, directed=True, indices=int(np.ravel_multi_index(tuple(seed), passable.shape)))
    t_search = time.perf_counter() - t0
    return t_graph, t_search, np.where(np.isfinite(d), d, plan.INF).astype(np.int64).reshape(passable.shape), graph.nnz


def measure(n, reps):
    voxel = 8.0 / n
    vol = TSDFVolume([[0.0, (n - 1) * voxel]] * 3, voxel, device=DEV)
    assert vol.dims == (n, n, n), vol.dims
    vol.tsdf.copy_(torch.from_numpy(room(n)))
    vol.weight.fill_(1.0)
    field = vol.esdf(1.0)
    start = [c * voxel for c in (n // 8, n // 4, 7 * n // 8)]
    goal = [c * voxel for c in (7 * n // 8, n // 2, n // 8)]
    field.plan(start, goal, robot_radius=RADIUS)            # warm-up
    rec = {"brick": list(plan.brick()), "lattice": [n, n, n], "voxel": voxel, "robot_radius": RADIUS,
           "sweep_batch": plan.SWEEP_BATCH}
    p_ms, p_wall, p_res = timed(lambda: field.plan(start, goal, robot_radius=RADIUS), reps)
    r_ms, r_wall, r_res = timed(lambda: field.reachable([start], robot_radius=RADIUS), reps)
    res = p_res[-1]
    assert res["reachable"] and all(torch.equal(r["cells"], res["cells"]) for r in p_res)
    assert all(torch.equal(r, r_res[0]) for r in r_res)
    rec["plan"] = {"ms_kernels": sum(statistics.median(p_ms[k]) for k in KERNELS),
                   "s_wall": statistics.median(p_wall), "sweeps": [r["sweeps"] for r in p_res],
                   "length_m": res["length_m"], "min_clearance_m": res["min_clearance_m"],
                   "path_cells": int(res["cells"].shape[0]), "s_wall_all": p_wall}
    rec["reachable"] = {"ms_kernels": sum(statistics.median(r_ms[k]) for k in KERNELS),
                        "s_wall": statistics.median(r_wall), "cells_reached": int(r_res[0].sum()), "s_wall_all": r_wall}
    for k in KERNELS:
        rec["plan"][f"ms_{k}_kernel"], rec["plan"][f"ms_{k}_kernel_all"] = statistics.median(p_ms[k]), p_ms[k]
        rec["reachable"][f"ms_{k}_kernel"], rec["reachable"][f"ms_{k}_kernel_all"] = statistics.median(r_ms[k]), r_ms[k]
    # the sweeps of the field alone, and the share of workgroups that found their brick dirty
    passable = field.passable(RADIUS)
    g = plan.geodesic_field(passable, [res["goal_cell"]])
    rec["plan"]["sweeps_field"] = g.sweeps
    rec["passable_share"] = float((passable != 0).double().mean())
    return rec, field, passable, res, g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--also", nargs="*", default=[])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "geodesic.json"))
    a = ap.parse_args()
    rec, field, passable, res, g = measure(a.n, a.reps)
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, **rec}
    print(json.dumps({k: v for k, v in out.items()}), flush=True)
    if not a.no_host:
        p = passable.cpu().numpy() != 0
        t_graph, t_search, d, nnz = host_dijkstra(p, res["goal_cell"])
        out["host"] = {"s_scipy_graph_build_wall": t_graph, "s_scipy_dijkstra_wall": t_search, "graph_edges": int(nnz),
                       "field_equals_host_dijkstra": bool(np.array_equal(d, g.cost.cpu().numpy().astype(np.int64)))}
        print(json.dumps(out["host"]), flush=True)
    if a.also:
        out["bricks"] = {}
        for lib in a.also:
            tmp = os.path.abspath(a.out) + ".child"
            env = dict(os.environ, GOSLAM_HIP_LIB=os.path.abspath(lib))
            subprocess.run([sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--n", str(a.n), "--no-host",
                            "--out", tmp], env=env, check=True, timeout=300)
            with open(tmp) as fh:
                child = json.load(fh)
            os.remove(tmp)
            out["bricks"][os.path.basename(lib)] = {k: child[k] for k in ("brick", "plan", "reachable")}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
