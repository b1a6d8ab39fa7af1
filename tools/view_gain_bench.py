"""View gain on one GPU, written to profiles/view_gain.json:
    timeout -k 10 900 python tools/view_gain_bench.py [--reps 5] [--n 256] [--no-host] [--also LIB ...] [--out FILE]
The n^3 half-seen room of tools/frontier_bench.py (8 m, a wall with one door, nothing observed beyond the wall), its
distance field built with max_distance 1 m.  A robot of 0.25 m starts where tools/geodesic_bench.py starts; the candidates
are `ESDF.view_candidates`' at the default stride on the five layers of axis 1 around the start's, cut at the default 4096;
each is looked from at 8 headings with a 90 x 60 degree camera of 96 x 64 rays and a range of 64 cells.  Medians of --reps
runs of
  `view.gain_table`, the 8 gs_view_gain calls alone: the kernel's own time summed over the headings (library kernel
  timer: view_gain, and view_pack in a build that has it) and the wall time;
  `ESDF.next_view`, which adds passability, snapping, the cost-to-go field, the candidates, the read and the walk.
Unless --no-host, the serial restatement (tests/view_gain_restatement.py) walks the first --host-views candidates at
heading 0 on the host: its seconds and whether its counts equal the kernel's.  It is one thread of an interpreter on
another processor: the number is recorded, no ratio is claimed.  Nothing earlier computes a view gain on the GPU, so there
is no other comparator.

--also: further builds of the library, each measured in a child process of its own (GOSLAM_HIP_LIB) and recorded under
"builds" by the library's file name, with whether its table equals this one's.  Such a build is csrc/view_gain.hip
compiled with the Makefile's flags plus -DVIEW_READ_FIRST=1 (read the mask's word first and skip the atomic OR when the
bit is already set), -DVIEW_PACKED=1 (the walk reads a 2-bit copy of `state` that a pre-pass packs, 16 cells to a word) or
-DVIEW_THREADS=256 / 512 (smaller workgroups), linked with the other objects of csrc/ into a shared library of another
name; `make -C go_slam_amd/csrc view_variants` builds the four of DESIGN section 27's table as libgoslam_hip_view_readfirst.so,
_packed.so, _t512.so and _t256.so, and giving the shipped library between them measures it the same way (A B A B)."""
import argparse
import ctypes
import hashlib
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
from go_slam_amd import _lib, view                                 # noqa: E402
from go_slam_amd.tsdf import TSDFVolume                            # noqa: E402
import geodesic_bench                                              # noqa: E402  (its room)

DEV = "cuda:0"
KERNELS = ("view_gain", "view_pack", "geodesic_fill", "geodesic_seed", "geodesic_relax", "geodesic_path")
RADIUS = 0.25
CAMERA = {"hfov_deg": 90.0, "vfov_deg": 60.0, "n_u": 96, "n_v": 64, "pitch_deg": 0.0}
N_YAW, RANGE_CELLS, UP_AXIS = 8, 64, 1


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
    return rec


def measure(n, reps):
    voxel = 8.0 / n
    vol = TSDFVolume([[0.0, (n - 1) * voxel]] * 3, voxel, device=DEV)
    assert vol.dims == (n, n, n), vol.dims
    vol.tsdf.copy_(torch.from_numpy(geodesic_bench.room(n)))
    vol.weight.fill_(1.0)
    vol.weight[n // 2 + 1:] = 0.0                           # never observed beyond the wall
    field = vol.esdf(1.0)
    start = [c * voxel for c in (n // 8, n // 4, 7 * n // 8)]
    height = ((n // 4 - 2) * voxel, (n // 4 + 2) * voxel)
    camera = dict(CAMERA, range_m=RANGE_CELLS * voxel)
    cells, cost, _ = field.view_candidates(start, UP_AXIS, height, robot_radius=RADIUS)
    range_cells, heads = view.headings(view.camera_arguments(camera, "view_gain_bench"), N_YAW, UP_AXIS, voxel,
                                       "view_gain_bench")
    assert range_cells == RANGE_CELLS
    L = _lib.lib()
    boxes = [list(box) for _, _, box in heads]
    rec = {"lattice": [n, n, n], "voxel": voxel, "robot_radius": RADIUS, "camera": camera, "n_yaw": N_YAW,
           "range_cells": range_cells, "n_candidates": int(cells.shape[0]), "n_rays": CAMERA["n_u"] * CAMERA["n_v"],
           "boxes": boxes, "box_cells": [view._box_cells(b) for b in boxes],
           "lds_bytes": [int(L.gs_view_gain_lds_bytes((ctypes.c_int * 6)(*b))) for b in boxes]}
    view.gain_table(field.state, cells, heads, range_cells, 0)                   # warm-up
    g_ms, g_wall, g_res = timed(lambda: view.gain_table(field.state, cells, heads, range_cells, 0), reps)
    table = g_res[-1]
    assert all(torch.equal(r, table) for r in g_res)
    host = table.cpu().numpy()
    rec["gain_table"] = {**record(g_ms, g_wall), "table_sha256": hashlib.sha256(host.tobytes()).hexdigest(),
                         "cells_counted": int(host[:, :, 3].sum()), "unknown_counted": int(host[:, :, 0].sum()),
                         "largest_gain_cells": int(host[:, :, 0].max())}
    kw = dict(n_yaw=N_YAW, robot_radius=RADIUS)
    field.next_view(start, camera, UP_AXIS, height, **kw)
    n_ms, n_wall, n_res = timed(lambda: field.next_view(start, camera, UP_AXIS, height, **kw), reps)
    res = n_res[-1]
    assert all(r["view_cell"] == res["view_cell"] and r["yaw_index"] == res["yaw_index"] for r in n_res)
    rec["next_view"] = {**record(n_ms, n_wall), "view_cell": res["view_cell"], "yaw_index": res["yaw_index"],
                        "gain_cells": res["gain_cells"], "gain_m3": res["gain_m3"], "length_m": res["length_m"],
                        "n_qualified": res["n_qualified"], "path_cells": int(res["cells"].shape[0])}
    return rec, field, cells, heads, host


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--host-views", type=int, default=2)
    ap.add_argument("--also", nargs="*", default=[])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "view_gain.json"))
    a = ap.parse_args()
    rec, field, cells, heads, table = measure(a.n, a.reps)
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, **rec}
    print(json.dumps(out), flush=True)
    if not a.no_host:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import view_gain_restatement as VR
        state = field.state.cpu().numpy()
        some = cells[:a.host_views].cpu().numpy()
        t0 = time.perf_counter()
        want = VR.gains(state, some, heads[0][1], RANGE_CELLS * RANGE_CELLS, 0)
        t = time.perf_counter() - t0
        out["host"] = {"views": int(len(some)), "heading": 0, "s_restatement_wall": t,
                       "counts_equal_kernel": bool(np.array_equal(want.astype(np.int64), table[:len(some), 0]))}
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
            name = os.path.basename(lib)                    # a library given twice is measured twice: A B A B
            name += f"#{sum(k.split('#')[0] == name for k in out['builds']) + 1}" if name in out["builds"] else ""
            out["builds"][name] = {
                "gain_table": child["gain_table"], "next_view": child["next_view"], "lds_bytes": child["lds_bytes"],
                "table_equal": child["gain_table"]["table_sha256"] == out["gain_table"]["table_sha256"]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
