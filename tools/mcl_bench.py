"""The particle filter's kernels on one GPU, written to profiles/mcl.json:
    python tools/mcl_bench.py [--reps 20] [--out profiles/mcl.json] [--step-timeout 300]
The two floor plans of tools/scan_bench.py at 0.05 m, 400 x 400 and 1024 x 1024 cells, a scan of 360 beams cast on the
map itself, 360 headings, particles seeded one cell around the pose the scan was cast from.  Each map is measured in a
child process of its own under a time limit; the first one that fails ends the run.  Per map and N in {512, 4096, 65536},
medians of --reps runs of
  mcl_move, mcl_weigh, mcl_estimate, mcl_resample   the kernels' own times (library kernel timer), on device-resident inputs;
  with mcl_weigh the gathers N * B', one byte each, and the bytes per second they come to -- to set beside the window
  search of section 36 that a tick replaces (0.58 to 0.75 ms, 1.13 to 1.44 TB/s) and the 16.8-18.8 TB/s at which the
  guide's gather kernel reads rows out of the L2s;
  tick_wall_ms   one `ParticleFilter.tick` from the host's side: beam_ends in numpy, the upload of its [H,B',2] table, the
                 noise, the three or four launches and the one read of sixteen words;
and, once, the wall time of tests/mcl_restatement.py's tick on the host for the closed loop's first tick (48 x 40, 60
beams, 512 particles), with whether the kernels' tick equals it.  The host restatement is Python and numpy on one thread:
the numbers are recorded, no ratio to it is claimed.  No other form of the weigh kernel was built, so there is no
--also here."""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from scan_bench import DEV, L2_GATHER_TBPS, MAPS, RES, floor_plan, kernel_ms      # noqa: E402

N_HEADINGS, N_BEAMS = 360, 360
PARTICLES = (512, 4096, 65536)


def measure(name, reps):
    import numpy as np
    import torch
    from go_slam_amd import mcl as M
    from go_slam_amd import scan as S
    n = MAPS[name]
    host = floor_plan(n)
    cells = torch.from_numpy(host).to(DEV)
    grid = {"cells": cells, "origin": (0.0, 0.0), "resolution": RES}
    free = np.argwhere(host[n // 4:3 * n // 4, n // 4:3 * n // 4] == 254) + n // 4
    cell = tuple(int(v) for v in free[len(free) // 3])
    k_true = 77
    xy = ((cell[0] + 0.5) * RES, (cell[1] + 0.5) * RES)
    yaw = 2.0 * math.pi * k_true / N_HEADINGS
    scan = S.scan_on_map(grid, xy, yaw, N_BEAMS, 360.0, 12.0)
    ranges, angles = scan["ranges_m"].cpu().numpy(), scan["angles"]
    rec = {"map": [n, n], "resolution": RES, "headings": N_HEADINGS, "beams_cast": N_BEAMS, "pose": [cell[0], cell[1], k_true],
           "particles": {}}
    for N in PARTICLES:
        pf = M.ParticleFilter(grid, N, N_HEADINGS, n_beams=N_BEAMS, max_range=12.0, seed=N)
        pf.seed_around(xy, yaw, RES, 2.0 * math.pi / N_HEADINGS)
        ends = torch.from_numpy(M.beam_ends(ranges, angles, N_HEADINGS, RES, 0.0, 12.0)).to(DEV)
        B = int(ends.shape[1])
        noise = M.motion_noise(N, (100, 50, 1), pf.generator)
        start = pf.particles.clone()
        moved = torch.empty_like(start)
        S_, best, w, cum, stats = pf._out
        cap = pf.R * pf.R + 1
        M.move(start, pf.rot, noise, (200, 0, 1), pf.shape, out=moved)              # warm-up of all four
        M.weigh(pf.cost, pf.cells, moved, ends, cap, out=(S_, best))
        M.estimate(S_, moved, pf.rot, pf.lut, out=(w, cum, stats))
        m = M.moments(stats.cpu().tolist())
        fresh = torch.empty_like(start)
        q = (0x9e3779b9 * m["W"]) >> 32
        M.resample(cum, moved, m["W"], q, out=fresh)
        torch.cuda.synchronize()
        times = {"mcl_move": kernel_ms(lambda: M.move(start, pf.rot, noise, (200, 0, 1), pf.shape, out=moved), "mcl_move", reps),
                 "mcl_weigh": kernel_ms(lambda: M.weigh(pf.cost, pf.cells, moved, ends, cap, out=(S_, best)), "mcl_weigh", reps),
                 "mcl_estimate": kernel_ms(lambda: M.estimate(S_, moved, pf.rot, pf.lut, out=(w, cum, stats)), "mcl_estimate", reps),
                 "mcl_resample": kernel_ms(lambda: M.resample(cum, moved, m["W"], q, out=fresh), "mcl_resample", reps)}
        walls, resampled = [], 0
        for _ in range(reps):
            pf.seed_around(xy, yaw, RES, 2.0 * math.pi / N_HEADINGS)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            est = pf.tick((0, 0, 0), ranges, angles, (100, 50, 1))
            torch.cuda.synchronize()
            walls.append((time.perf_counter() - t0) * 1e3)
            resampled += est["resampled"]
        ms = statistics.median(times["mcl_weigh"])
        gathers = m["standing"] * B
        rec["particles"][str(N)] = {
            "valid_beams": B, "standing": m["standing"], "with_weight": m["positive"], "ess": m["W"] ** 2 / m["W2"],
            "best_mean_cost": (m["best"] >> 32) / B, **{f"ms_{k}": statistics.median(v) for k, v in times.items()},
            **{f"ms_{k}_all": v for k, v in times.items()}, "gathers": gathers, "gathered_bytes_per_s": gathers / (ms / 1e3),
            "fraction_of_l2_gather_rate": [gathers / (ms / 1e3) / (x * 1e12) for x in L2_GATHER_TBPS],
            "tick_wall_ms": statistics.median(walls), "tick_wall_ms_all": walls, "ticks_resampled": resampled,
            "tick_error_cells": math.hypot(est["xy"][0] - xy[0], est["xy"][1] - xy[1]) / RES if est["found"] else None}
        del pf
    rec["device"] = torch.cuda.get_device_name(0)
    if name == "plan400":
        import mcl_restatement as R
        import test_mcl_cpu as MC
        cells_s, cost_s, rot, lut = MC.loop_tables()
        rng = np.random.default_rng(0)
        start = np.rint(np.array(MC.LOOP_START) + rng.standard_normal((MC.LOOP_N, 3)) * np.array(MC.LOOP_SEED_SIGMAS))
        start[:, 2] %= MC.LOOP_H
        start = start.astype(np.int32)
        noise = np.rint(rng.standard_normal((MC.LOOP_N, 3)) * np.array(MC.LOOP_SIGMAS)).astype(np.int32)
        ends = MC.loop_ends(0)
        t0 = time.perf_counter()
        want, info = R.tick(start, MC.LOOP_ROUTE[0], noise, ends, cost_s, cells_s, rot, lut, MC.LOOP_R ** 2 + 1, False,
                            lambda: 0x9e3779b9)
        rec["s_host_restatement_tick_48x40_60_beams_512_particles"] = time.perf_counter() - t0
        dev = lambda a: torch.from_numpy(np.array(a)).to(DEV)                      # noqa: E731
        p = M.move(dev(start), rot, noise, MC.LOOP_ROUTE[0], cells_s.shape)
        S_, best = M.weigh(dev(cost_s), dev(cells_s), p, ends, MC.LOOP_R ** 2 + 1)
        w, cum, stats = M.estimate(S_, p, rot, lut)
        words = [v & ((1 << 64) - 1) for v in stats.cpu().tolist()]
        got = M.resample(cum, p, words[0], (0x9e3779b9 * words[0]) >> 32) if info["resampled"] else p
        rec["equals_host_restatement"] = bool(words == info["stats"] and np.array_equal(got.cpu().numpy(), want))
    return rec


def child(name, reps, timeout):
    cmd = [sys.executable, os.path.abspath(__file__), "--one", name, "--reps", str(reps)]
    try:
        res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        print(f"{name}: no result within {timeout} s; stopping", flush=True)
        return None
    lines = [l for l in res.stdout.splitlines() if l.startswith("RECORD ")]
    if res.returncode != 0 or not lines:
        print(f"{name}: exit status {res.returncode}; stopping\n{res.stdout[-3000:]}", flush=True)
        return None
    return json.loads(lines[-1][len("RECORD "):])


def brief(rec):
    return {k: ({n: {m: v for m, v in r.items() if not m.endswith("_all")} for n, r in val.items()} if k == "particles" else val)
            for k, val in rec.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mcl.json"))
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--one", choices=sorted(MAPS), help="measure this map in this process and print its record")
    a = ap.parse_args()
    if a.one:
        print("RECORD " + json.dumps(measure(a.one, a.reps)), flush=True)
        return 0
    out = {"reps": a.reps, "l2_gather_TBps_of_the_guide": list(L2_GATHER_TBPS),
           "window_search_of_section_36": {"ms": [0.58, 0.75], "gathered_TBps": [1.13, 1.44]}, "maps": {}}
    for name in MAPS:                                       # a fresh child per map; the parent never opens the GPU
        rec = child(name, a.reps, a.step_timeout)
        if rec is None:
            return 1
        out["device"] = rec.pop("device")
        out["maps"][name] = rec
        print(json.dumps({name: brief(rec)}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
