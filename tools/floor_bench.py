"""Drivable-floor map of a state lattice on one GPU, written to profiles/floor.json:
    python tools/floor_bench.py [--reps 20] [--out profiles/floor.json] [--step-timeout 300]
Two lattices: the 128^3 door room of tools/geodesic_bench.py (8 m, a solid shell, a wall with one door) and a
512 x 512 x 128 room of the same make at 1/16 m.  Each is measured in a child process of its own under a time limit; the
first one that fails ends the run.  Per lattice and up axis 0, 1 and 2, medians of --reps runs of the kernels' own times
(library kernel timer) of
  floor_columns    band: the positions 1 .. 16, headroom 8 cells (a robot of 0.5 m); with it the state bytes of the whole
                   window [0, 23] of every column, the bytes a walk must read (it ends at the first stand's headroom) and
                   the bytes per second either comes to;
  floor_footprint  R2 = 16 (a disc of 0.25 m) and R2 = 1024 (the cap of the halo), S = 1;
  esdf_slice       the existing kernel over the slab of the same 16 layers: it reads the same state bytes and the int32
                   and float32 fields beside them;
and the wall time of tests/floor_restatement.py on the host for the same arguments (the large lattice: up axis 2 only),
with whether its maps equal the kernels'.  The host restatement is numpy on one thread: the numbers are recorded, no
ratio to it is claimed."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

DEV = "cuda:0"
LATTICES = {"room128": ((128, 128, 128), 8.0 / 128), "room512x512x128": ((512, 512, 128), 1.0 / 16)}
BAND, H, S = (1, 16), 8, 1
R2S = (16, 1024)


def room(dims):
    """tsdf float32 [dims]: -1 in the shell and in a wall across axis 0 with one door, +1 elsewhere (geodesic_bench's)."""
    import numpy as np
    n0, n1, n2 = dims
    t = np.ones(dims, dtype=np.float32)
    t[0], t[-1], t[:, 0], t[:, -1], t[:, :, 0], t[:, :, -1] = -1, -1, -1, -1, -1, -1
    t[n0 // 2 - 1:n0 // 2 + 1] = -1
    t[n0 // 2 - 1:n0 // 2 + 1, 1:3 * n1 // 4, 7 * n2 // 16:9 * n2 // 16] = 1
    return t


def kernel_ms(fn, name, reps):
    import torch
    from go_slam_amd import _lib
    out = []
    for _ in range(reps):
        with _lib.kernel_timer(DEV) as kt:
            fn()
            torch.cuda.synchronize()
        out.append(kt.read()[name][0])
    return out


def measure(name, reps):
    import numpy as np
    import torch
    import floor_restatement as R
    from go_slam_amd import floor as F
    from go_slam_amd.tsdf import TSDFVolume
    dims, voxel = LATTICES[name]
    vol = TSDFVolume([[0.0, (n - 1) * voxel] for n in dims], voxel, device=DEV)
    assert vol.dims == dims, vol.dims
    vol.tsdf.copy_(torch.from_numpy(room(dims)))
    vol.weight.fill_(1.0)
    field = vol.esdf(1.0)
    host_state = field.state.cpu().numpy()
    rec = {"lattice": list(dims), "voxel": voxel, "band": list(BAND), "H": H, "S": S, "axes": {}}
    for a in (0, 1, 2):
        n_a = dims[a]
        cols = int(np.prod(dims)) // n_a
        height = (field.lo[a] + (BAND[0] - 0.5) * voxel, field.lo[a] + (BAND[1] + 0.5) * voxel)
        assert field.slice_arguments(a, height)[1:3] == BAND
        floor, kind = F.columns(field.state, a, 1, BAND[0], BAND[1], H)               # warm-up
        t_cols = kernel_ms(lambda: F.columns(field.state, a, 1, BAND[0], BAND[1], H, out=(floor, kind)), "floor_columns", reps)
        t_slice = kernel_ms(lambda: field.occupancy_slice(a, height), "esdf_slice", reps)
        jstart, jend = max(BAND[0] - 1, 0), min(BAND[1] + H - 1, n_a - 1)
        f, k = floor.cpu().numpy().astype(np.int64), kind.cpu().numpy()
        walked = np.where(f >= 0, np.minimum(f + H - 1, jend) - jstart + 1, jend - jstart + 1)
        ax = {"columns": cols, "kinds": [int((k == v).sum()) for v in range(4)],
              "ms_floor_columns": statistics.median(t_cols), "ms_floor_columns_all": t_cols,
              "ms_esdf_slice": statistics.median(t_slice), "ms_esdf_slice_all": t_slice,
              "window_state_bytes": cols * (jend - jstart + 1), "must_read_state_bytes": int(walked.sum()),
              "esdf_slice_bytes": cols * (BAND[1] - BAND[0] + 1) * 9}
        sec = ax["ms_floor_columns"] / 1e3
        ax["window_bytes_per_s"] = ax["window_state_bytes"] / sec
        ax["must_read_bytes_per_s"] = ax["must_read_state_bytes"] / sec
        ax["esdf_slice_bytes_per_s"] = ax["esdf_slice_bytes"] / (ax["ms_esdf_slice"] / 1e3)
        ax["columns_over_esdf_slice"] = ax["ms_floor_columns"] / ax["ms_esdf_slice"]
        maps = {}
        for R2 in R2S:
            maps[R2] = F.footprint(floor, kind, R2, S)                                   # warm-up
            t = kernel_ms(lambda: F.footprint(floor, kind, R2, S, out=maps[R2]), "floor_footprint", reps)
            ax[f"ms_floor_footprint_R2_{R2}"], ax[f"ms_floor_footprint_R2_{R2}_all"] = statistics.median(t), t
        if name == "room128" or a == 2:
            t0 = time.perf_counter()
            want = R.columns(host_state, a, 1, BAND[0], BAND[1], H)
            ax["s_host_restatement_columns"] = time.perf_counter() - t0
            t0 = time.perf_counter()
            want_map = R.footprint(want[0], want[1], R2S[0], S)
            ax["s_host_restatement_footprint_R2_16"] = time.perf_counter() - t0
            ax["equals_host_restatement"] = bool(
                np.array_equal(want[0], floor.cpu().numpy()) and np.array_equal(want[1], k)
                and all(np.array_equal(w, g.cpu().numpy()) for w, g in zip(want_map, maps[R2S[0]])))
        rec["axes"][str(a)] = ax
    ms = [rec["axes"][str(a)]["ms_floor_columns"] for a in (0, 1, 2)]
    rec["columns_axis_spread"] = max(ms) / min(ms)
    rec["device"] = torch.cuda.get_device_name(0)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "floor.json"))
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--one", choices=sorted(LATTICES), help="measure this lattice in this process and print its record")
    a = ap.parse_args()
    if a.one:
        print("RECORD " + json.dumps(measure(a.one, a.reps)), flush=True)
        return 0
    out = {"reps": a.reps, "lattices": {}}
    for name in LATTICES:                                   # a fresh child per lattice; the parent never opens the GPU
        try:
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", name, "--reps", str(a.reps)],
                                 stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.step_timeout)
        except subprocess.TimeoutExpired:
            print(f"{name}: no result within {a.step_timeout} s; stopping", flush=True)
            return 1
        lines = [l for l in res.stdout.splitlines() if l.startswith("RECORD ")]
        if res.returncode != 0 or not lines:
            print(f"{name}: exit status {res.returncode}; stopping\n{res.stdout[-3000:]}", flush=True)
            return 1
        rec = json.loads(lines[-1][len("RECORD "):])
        out["device"] = rec.pop("device")
        out["lattices"][name] = rec
        print(json.dumps({name: {k: ({ax: {m: v for m, v in r.items() if not m.endswith("_all")} for ax, r in val.items()}
                                     if k == "axes" else val) for k, val in rec.items()}}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
