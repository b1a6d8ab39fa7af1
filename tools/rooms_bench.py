"""Rooms and doorways on one GPU, written to profiles/rooms.json:
    timeout -k 10 900 python tools/rooms_bench.py [--reps 5] [--n 256] [--out FILE]
A hand-built flat on an n^3 lattice over 8 m: a solid shell, one wall across the middle of x and one across the middle of z
in each half, which makes four rooms, and a door 1 m wide and 2 m high in each of the three walls; its distance field built
with max_distance 1 m.  With a robot of 0.25 m and a core radius of 0.6 m (no door lets a ball of that radius through),
medians of --reps runs of `ESDF.rooms`: every stage's kernels' own times (library kernel timer, a relaxation summed over its
sweeps), the wall time of the call, the sweeps of each of the four relaxations, and what was found.  Nothing here has been
measured before and no target is set.  The one comparison worth reading is ms_room_relax_kernel and sweeps["rooms"] beside
ms_geodesic_relax_kernel and sweeps["cost"]: both relaxations walk the same wavefront over the same lattice, the second
one with the costs already there."""
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
from go_slam_amd import _lib, frontier, rooms                      # noqa: E402
from go_slam_amd.tsdf import TSDFVolume                            # noqa: E402

DEV = "cuda:0"
STAGES = {"cores": ("room_mark", "frontier_relax", "frontier_count", "frontier_scan", "room_emit", "room_sizes",
                    "room_seed"),
          "cost": ("geodesic_fill", "geodesic_seed", "geodesic_relax"),
          "rooms": ("room_relax",),
          "doors": ("room_door_mark",),
          "tables": ("room_table_init", "room_table", "room_door_table_init", "room_door_table")}
KERNELS = tuple(k for stage in STAGES.values() for k in stage)
RADIUS, CORE_RADIUS = 0.25, 0.6


def flat(n):
    """float32 [n,n,n]: +1 in free space, -1 in the shell, the three walls and outside their doors."""
    t = np.ones((n, n, n), dtype=np.float32)
    t[0], t[-1], t[:, 0], t[:, -1], t[:, :, 0], t[:, :, -1] = -1, -1, -1, -1, -1, -1
    m, door, high = n // 2, max(n // 8, 2), max(n // 4, 2)              # doors 1 m wide, 2 m high, from the floor y = 1
    t[m:m + 2] = -1
    t[m:m + 2, 1:1 + high, n // 4:n // 4 + door] = 1
    t[:, :, m:m + 2] = -1
    t[n // 4:n // 4 + door, 1:1 + high, m:m + 2] = 1
    t[3 * n // 4:3 * n // 4 + door, 1:1 + high, m:m + 2] = 1
    t[m:m + 2, :, m:m + 2] = -1                                         # where the walls cross
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rooms.json"))
    a = ap.parse_args()
    n = a.n
    voxel = 8.0 / n
    vol = TSDFVolume([[0.0, (n - 1) * voxel]] * 3, voxel, device=DEV)
    assert vol.dims == (n, n, n), vol.dims
    vol.tsdf.copy_(torch.from_numpy(flat(n)))
    vol.weight.fill_(1.0)
    field = vol.esdf(1.0)
    field.rooms(robot_radius=RADIUS, core_radius=CORE_RADIUS)           # warm-up
    ms, wall, results = {k: [] for k in KERNELS}, [], []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        with _lib.kernel_timer(DEV) as kt:
            t0 = time.perf_counter()
            results.append(field.rooms(robot_radius=RADIUS, core_radius=CORE_RADIUS))
            torch.cuda.synchronize()
            wall.append(time.perf_counter() - t0)
        got = kt.read()
        for k in KERNELS:
            ms[k].append(got.get(k, (0.0, 0))[0])
    seg = results[-1]
    assert all(torch.equal(r.label, seg.label) and torch.equal(r.door_label, seg.door_label) for r in results)
    # frontier_relax, _count and _scan run for the cores and for the doorways: the timer sums both under "cores"
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "brick": list(frontier.brick()), "lattice": [n, n, n],
           "voxel": voxel, "robot_radius": RADIUS, "core_radius": CORE_RADIUS, "sweep_batch": rooms.SWEEP_BATCH,
           "s_wall": statistics.median(wall), "s_wall_all": wall,
           "sweeps": {k: [r.sweeps[k] for r in results] for k in ("cores", "cost", "rooms", "doors")},
           "n_rooms": seg.n_rooms, "n_doors": seg.n_doors, "counts": [int(v) for v in seg.counts.cpu().tolist()],
           "room_cells": seg.rooms["size"].cpu().tolist(), "door_cells": seg.doors["size"].cpu().tolist(),
           "door_width_m": seg.door_width_m.cpu().tolist(), "graph": seg.graph()["doors"]}
    for k in KERNELS:
        out[f"ms_{k}_kernel"], out[f"ms_{k}_kernel_all"] = statistics.median(ms[k]), ms[k]
    out["ms_stage_kernels"] = {s: sum(statistics.median(ms[k]) for k in ks) for s, ks in STAGES.items()}
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
