"""Range scans and the correlative scan match on one GPU, written to profiles/scan.json:
    python tools/scan_bench.py [--reps 10] [--out profiles/scan.json] [--step-timeout 300] [--also v1=PATH]
Two maps at 0.05 m: 400 x 400 and 1024 x 1024 cells of a floor plan (an occupied border, walls every 100 cells with a
door each, drawn boxes, an unknown strip).  Each is measured in a child process of its own under a time limit; the first
one that fails ends the run.  Per map, medians of --reps runs of the kernels' own times (library kernel timer) of
  scan_match  360 yaws x 360 beams of a scan cast on the map itself, over the whole map and over a window of 4 m around
              the pose (81 x 81 cells); the 1024 x 1024 whole-map search is two launches (2^28 candidates each at most) and
              their times are added.  With it the gathers Y * w_u * w_v * B, one byte each, and the bytes per second they
              come to -- to set beside the 16.8-18.8 TB/s at which the guide's gather kernel reads rows out of the L2s;
  scan_field  radius 6 and radius 15;
  scan_cast   1024 poses of 360 beams across the whole map;
whether the search found the pose the scan was cast from, and the wall time of tests/scan_restatement.py on the host for
the recovery scene of tests/test_scan_cpu.py (48 x 40, 32 yaws, 60 beams).  The host restatement is numpy on one thread:
the numbers are recorded, no ratio to it is claimed.
--also NAME=PATH measures scan_match again in a library built with another form of the kernel (same ABI; the child runs
with GOSLAM_HIP_LIB=PATH) and records it under "variants".  The one other form tried, the design the kernel started
from with one translation and one byte load per lane and beam, is csrc/scan.hip compiled with -DSCAN_MATCH_V4=0:
    python tools/scan_bench.py --build-variant v1      (writes go_slam_amd/csrc/libgoslam_hip_scan_v1.so)"""
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

DEV = "cuda:0"
MAPS = {"plan400": 400, "plan1024": 1024}
RES, N_YAW, N_BEAMS, WINDOW_M = 0.05, 360, 360, 2.0
L2_GATHER_TBPS = (16.8, 18.8)          # chip-wide, rows shared by every workgroup out of the XCDs' L2s
VARIANT_DEFS = {"v1": "-DSCAN_MATCH_V4=0"}


def floor_plan(n):
    """uint8 [n,n]: an occupied border, walls every 100 cells each way with a door of 16 cells in every span, 3 % of the
    8 x 8 blocks occupied, an unknown strip along one side."""
    import numpy as np
    rng = np.random.default_rng(n)
    c = np.full((n, n), 254, dtype=np.uint8)
    blocks = rng.random((n // 8 + 1, n // 8 + 1)) < 0.03
    c[np.kron(blocks, np.ones((8, 8), dtype=bool))[:n, :n]] = 0
    for w in range(100, n - 50, 100):
        c[w, :] = 0
        c[:, w] = 0
        for s in range(0, n, 100):
            d = s + int(rng.integers(20, 60))
            c[w, d:d + 16] = 254
            d = s + int(rng.integers(20, 60))
            c[d:d + 16, w] = 254
    c[0], c[-1], c[:, 0], c[:, -1] = 0, 0, 0, 0
    c[n - 12:, :] = 205
    return c


def kernel_ms(fn, name, reps):
    import torch
    from go_slam_amd import _lib
    out = []
    for _ in range(reps):
        with _lib.kernel_timer(DEV) as kt:
            fn()
            torch.cuda.synchronize()
        out.append(kt.read()[name][0])                      # the total over the launches of one call
    return out


def measure(name, reps, match_only=False):
    import numpy as np
    import torch
    from go_slam_amd import scan as S
    n = MAPS[name]
    host = floor_plan(n)
    cells = torch.from_numpy(host).to(DEV)
    grid = {"cells": cells, "origin": (0.0, 0.0), "resolution": RES}
    free = np.argwhere(host[n // 4:3 * n // 4, n // 4:3 * n // 4] == 254) + n // 4
    cell = tuple(int(v) for v in free[len(free) // 3])
    k_true = 77
    xy = ((cell[0] + 0.5) * RES, (cell[1] + 0.5) * RES)
    scan = S.scan_on_map(grid, xy, 2.0 * math.pi * k_true / N_YAW, N_BEAMS, 360.0, 12.0)
    ranges, angles = scan["ranges_m"].cpu().numpy(), scan["angles"]
    yaws = 2.0 * math.pi * np.arange(N_YAW) / N_YAW
    r = int(math.ceil(WINDOW_M / RES))
    windows = {"whole": None, "window_4m": (max(cell[0] - r, 0), max(cell[1] - r, 0), 2 * r + 1, 2 * r + 1)}
    rec = {"map": [n, n], "resolution": RES, "yaws": N_YAW, "beams_cast": N_BEAMS, "pose": [cell[0], cell[1], k_true],
           "match": {}}
    for key, window in windows.items():
        res = S.match_scan(grid, ranges, angles, yaws, window=window, max_range=12.0)   # warm-up
        t = kernel_ms(lambda: S.match_scan(grid, ranges, angles, yaws, window=window, max_range=12.0), "scan_match",
                      reps if key != "whole" or n <= 512 else max(reps // 3, 3))
        w = res["window"]
        gathers = N_YAW * w[2] * w[3] * res["n_beams"]
        ms = statistics.median(t)
        rec["match"][key] = {"window": list(w), "valid_beams": res["n_beams"], "ms": ms, "ms_all": t, "gathers": gathers,
                             "gathered_bytes_per_s": gathers / (ms / 1e3),
                             "fraction_of_l2_gather_rate": [gathers / (ms / 1e3) / (x * 1e12) for x in L2_GATHER_TBPS],
                             "best": [res["best"][0], list(res["best"][1])], "best_score": res["best_score"],
                             "found_the_pose": res["best"] == (k_true, cell)}
        del res
    rec["device"] = torch.cuda.get_device_name(0)
    if match_only:
        return rec
    for R_ in (6, 15):
        cost = S.field(cells, R_)
        t = kernel_ms(lambda: S.field(cells, R_, out=(cost,)), "scan_field", reps)
        rec[f"ms_scan_field_R{R_}"], rec[f"ms_scan_field_R{R_}_all"] = statistics.median(t), t
    rng = np.random.default_rng(1)
    poses = free[rng.integers(0, len(free), 1024)].astype(np.int32)
    dirs = S.beam_directions(angles, rng.random(1024) * 2.0 * math.pi)
    out = S.cast(cells, poses, dirs, min(2 * n * n, S.MAX_RANGE2))
    dirs_dev, poses_dev = torch.from_numpy(dirs).to(DEV), torch.from_numpy(poses).to(DEV)
    t = kernel_ms(lambda: S.cast(cells, poses_dev, dirs_dev, min(2 * n * n, S.MAX_RANGE2), out=out), "scan_cast", reps)
    rec["cast"] = {"poses": 1024, "beams": N_BEAMS, "ms": statistics.median(t), "ms_all": t,
                   "hits": int((out[0] == 1).sum()), "mean_range_cells": float(out[2][out[0] == 1].double().mean()) / 1000.0}
    if name == "plan400":
        import scan_restatement as R
        import test_scan_cpu as SC
        small = SC.scene()
        (c0, k0) = SC.SCENE_POSES[0]
        t0 = time.perf_counter()
        r_small, a_small, y_small = SC.scene_scan(c0, k0)
        rec["s_host_restatement_cast_60_beams"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        cost_small = R.field(small, SC.SCENE_R)
        rec["s_host_restatement_field_48x40_R6"] = time.perf_counter() - t0
        off = S.beam_offsets(r_small, a_small, y_small, 1.0, 0.0, float(SC.SCENE_RANGE))
        t0 = time.perf_counter()
        want = R.match(cost_small, small, off, (0, 0, 48, 40), SC.SCENE_R ** 2 + 1, False)
        rec["s_host_restatement_match_48x40_32_yaws"] = time.perf_counter() - t0
        got = S.match(S.field(torch.from_numpy(np.array(small)).to(DEV), SC.SCENE_R), torch.from_numpy(np.array(small)).to(DEV),
                      off, None, SC.SCENE_R ** 2 + 1)
        rec["equals_host_restatement"] = bool(np.array_equal(got[0].cpu().numpy(), want[0].view(np.int32))
                                              and (got[1].item() & 0xffffffffffffffff) == want[1])
    return rec


def build_variant(name):
    csrc = os.path.join(ROOT, "go_slam_amd", "csrc")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wall", "-Wno-unused-function",
             "-fno-gpu-rdc", "-munsafe-fp-atomics"]
    subprocess.run(["make", "-C", csrc, "-j8"], check=True)
    obj = os.path.join(csrc, f"scan.o.{name}")
    subprocess.run([hipcc] + flags + [VARIANT_DEFS[name], "-c", os.path.join(csrc, "scan.hip"), "-o", obj], check=True)
    others = sorted(os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".o") and f != "scan.o")
    lib = os.path.join(csrc, f"libgoslam_hip_scan_{name}.so")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib] + others + [obj], check=True)
    print(lib)
    return 0


def child(name, reps, timeout, lib=None):
    env = dict(os.environ, **({"GOSLAM_HIP_LIB": lib} if lib else {}))
    cmd = [sys.executable, os.path.abspath(__file__), "--one", name, "--reps", str(reps)] + (["--match-only"] if lib else [])
    try:
        res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout, env=env)
    except subprocess.TimeoutExpired:
        print(f"{name}: no result within {timeout} s; stopping", flush=True)
        return None
    lines = [l for l in res.stdout.splitlines() if l.startswith("RECORD ")]
    if res.returncode != 0 or not lines:
        print(f"{name}: exit status {res.returncode}; stopping\n{res.stdout[-3000:]}", flush=True)
        return None
    return json.loads(lines[-1][len("RECORD "):])


def brief(rec):
    return {k: ({w: {m: v for m, v in r.items() if not m.endswith("_all")} for w, r in val.items()} if k == "match" else val)
            for k, val in rec.items() if not k.endswith("_all") and k != "cast"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan.json"))
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--also", action="append", default=[], metavar="NAME=PATH")
    ap.add_argument("--build-variant", choices=sorted(VARIANT_DEFS))
    ap.add_argument("--one", choices=sorted(MAPS), help="measure this map in this process and print its record")
    ap.add_argument("--match-only", action="store_true")
    a = ap.parse_args()
    if a.build_variant:
        return build_variant(a.build_variant)
    if a.one:
        print("RECORD " + json.dumps(measure(a.one, a.reps, a.match_only)), flush=True)
        return 0
    out = {"reps": a.reps, "l2_gather_TBps_of_the_guide": list(L2_GATHER_TBPS), "maps": {}, "variants": {}}
    for name in MAPS:                                       # a fresh child per map; the parent never opens the GPU
        rec = child(name, a.reps, a.step_timeout)
        if rec is None:
            return 1
        out["device"] = rec.pop("device")
        out["maps"][name] = rec
        print(json.dumps({name: brief(rec)}), flush=True)
        for also in a.also:
            label, _, path = also.partition("=")
            rec = child(name, a.reps, a.step_timeout, os.path.abspath(path))
            if rec is None:
                return 1
            rec.pop("device")
            out["variants"].setdefault(label, {})[name] = rec["match"]
            print(json.dumps({f"{label}:{name}": brief(rec)["match"]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
