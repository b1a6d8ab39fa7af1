"""The sampled-rollout controller on one GPU, written to profiles/follow.json:
    timeout -k 10 600 python tools/follow_bench.py [--reps 20] [--n 128] [--no-host] [--out FILE]
One scene: tools/geodesic_bench.py's room split by a wall with one door on an n^3 lattice over 8 m, written straight into
a TSDFVolume, distance field built with max_distance 1 m; the robot (radius 0.25 m) moves in the plane of axes 0 and 2 a
quarter of the way up axis 1, from one room's corner to the other's.
Per K in {256, 2048, 16384} at T = 32, medians over --reps ticks of `Controller.step` from the start state (the nominal
sequence is reset before each, so every tick does the same work): the kernels' own times per launch (library kernel
timer: follow_rollouts, follow_weights, follow_update), their sum, and the wall time of the tick with its noise draw and
its one read; unless --no-host, the wall time of one tick of the numpy restatement (tests/follow_restatement.py) on the
host at the same K, the only comparator there is: no ratio is claimed.  Then one whole `Controller.drive` at K = 2048:
reached, ticks, length, clearance and wall time."""
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
from go_slam_amd import _lib, follow                               # noqa: E402
from go_slam_amd.tsdf import TSDFVolume                            # noqa: E402
from geodesic_bench import room                                    # noqa: E402  (tools/: beside this file)

DEV = "cuda:0"
KERNELS = ("follow_rollouts", "follow_weights", "follow_update")
ROLLOUTS = (256, 2048, 16384)
T, RADIUS = 32, 0.25


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "follow.json"))
    a = ap.parse_args()
    n = a.n
    voxel = 8.0 / n
    vol = TSDFVolume([[0.0, (n - 1) * voxel]] * 3, voxel, device=DEV)
    assert vol.dims == (n, n, n), vol.dims
    vol.tsdf.copy_(torch.from_numpy(room(n)))
    vol.weight.fill_(1.0)
    field = vol.esdf(1.0)
    start = [c * voxel for c in (n // 8, n // 4, 7 * n // 8)]
    goal = [c * voxel for c in (7 * n // 8, n // 4, n // 8)]
    state = [start[0], start[2], 1.0, 0.0]
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "lattice": [n, n, n], "voxel": voxel, "T": T,
           "robot_radius": RADIUS, "ticks": {}}
    for K in ROLLOUTS:
        ctl = follow.Controller(field, goal, 1, start[1], RADIUS, K=K, T=T, seed=0)
        ctl.step(state)                                                           # warm-up
        ms, wall = {k: [] for k in KERNELS}, []
        for _ in range(a.reps):
            ctl.reset()
            torch.cuda.synchronize()
            with _lib.kernel_timer(DEV) as kt:
                t0 = time.perf_counter()
                ctl.step(state)
                torch.cuda.synchronize()
                wall.append(time.perf_counter() - t0)
            got = kt.read()
            for k in KERNELS:
                ms[k].append(got[k][0])
        rec = {f"ms_{k}_kernel": statistics.median(ms[k]) for k in KERNELS}
        rec["ms_kernels"] = sum(rec.values())
        rec["ms_wall_tick"] = 1e3 * statistics.median(wall)
        rec.update({f"ms_{k}_kernel_all": ms[k] for k in KERNELS})
        if not a.no_host:
            import follow_restatement as R
            w = ctl.m["weights"]
            model = R.Model(ctl.dist.cpu().numpy(), ctl.togo.cpu().numpy(), field.lo, voxel, 1, start[1], ctl.m["dt"],
                            ctl.m["v_max"], ctl.m["w_max"], RADIUS, w["margin"], w["togo"], w["clear"], w["turn"], w["end"],
                            w["collision"])
            loop = R.Loop(model, K, T, ctl.sigma, ctl.lam, 0)
            t0 = time.perf_counter()
            loop.tick(state)
            rec["ms_restatement_tick_host"] = 1e3 * (time.perf_counter() - t0)
        out["ticks"][str(K)] = rec
        print(json.dumps({K: {k: v for k, v in rec.items() if not k.endswith("_all")}}), flush=True)
    ctl = follow.Controller(field, goal, 1, start[1], RADIUS, K=2048, T=T, seed=0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = ctl.drive(state, max_ticks=600)
    torch.cuda.synchronize()
    out["drive"] = {"K": 2048, "s_wall": time.perf_counter() - t0,
                    **{k: res[k] for k in ("reached", "ticks", "length_m", "min_clearance_m", "stops", "ess_min")}}
    print(json.dumps({"drive": out["drive"]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
