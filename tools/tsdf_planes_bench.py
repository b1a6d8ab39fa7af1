"""Plane finding on one GPU, written to profiles/tsdf_planes.json:
    timeout -k 10 900 python tools/tsdf_planes_bench.py [--reps 5] [--n 256 512] [--out profiles/tsdf_planes.json]
Per n, a room-sized volume (n^3 points over 8 m) fused from 16 frames of synth's arc over its wall and floor at 480 x 640,
in a world tilted by 20 degrees of roll and 10 of pitch.
  The kernels' own time (library kernel timer) of gs_tsdf_plane_votes at 16 bins, of gs_tsdf_plane_offsets along the
  directions `find_planes` found and along 16, and of gs_tsdf_plane_moments (the gather and the chunk sum) for the planes
  found and for 16.  Beside each the time a plain read of the tsdf and weight lattices (8 bytes per point) would take at
  6.29 TB/s, the rate a float4 copy reaches on this GPU's HBM: every kernel has to look at both lattices once, and most
  cells leave after their eight weights or eight values.
  The wall time of one `find_planes` and of one `upright` (a `find_planes`, the union lattice and one gs_tsdf_merge).
No parent commit finds planes: there is no ratio against one.  Medians of --reps windows of 10 launches."""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"
H, W = 480, 640
INTR = (577.590698, 578.729797, 318.905426, 242.683609)
K = 16
LAUNCHES = 10                    # per timed window
HBM_COPY_RATE = 6.29e12          # bytes per second, measured float4 copy
EXTENT = 8.0
LO = (-4.0, -4.0, -2.0)


def tilt():
    """float64 [4,4], the scene's world to the tilted one: 10 degrees about x, then 20 about z, about the box's middle."""
    import numpy as np
    a, b = math.radians(20.0), math.radians(10.0)
    Rz = np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1.0]])
    Rx = np.array([[1.0, 0, 0], [0, math.cos(b), -math.sin(b)], [0, math.sin(b), math.cos(b)]])
    c = np.array(LO) + 0.5 * EXTENT
    M = np.eye(4)
    M[:3, :3] = Rz @ Rx
    M[:3, 3] = c - M[:3, :3] @ c
    return M


def scene(n):
    import numpy as np
    import torch
    from go_slam_amd import synth
    from go_slam_amd.tsdf import TSDFVolume, w2c_matrices
    voxel = EXTENT / n
    poses = synth.arc_poses(K).to(DEV)
    disp = synth.plane_disps(poses, torch.tensor(INTR, device=DEV), H, W)
    depth = torch.where(disp > 0, 1.0 / disp, torch.zeros_like(disp)).contiguous()
    M = tilt()
    Minv = np.linalg.inv(M)
    w2c = torch.from_numpy(np.stack([(np.vstack([m, [0, 0, 0, 1.0]]) @ Minv)[:3, :]
                                     for m in w2c_matrices(poses).double().cpu().numpy()]))
    vol = TSDFVolume([[l, l + (n - 1) * voxel] for l in LO], voxel, device=DEV)
    assert vol.dims == (n, n, n), vol.dims
    vol.integrate(depth, w2c, INTR)
    return vol, M[:3, :3] @ np.array([0.0, -1.0, 0.0])


def windows(fn, names, reps):
    """Medians over `reps` windows of LAUNCHES calls of fn(): ms per call of each kernel of `names`."""
    import torch
    from go_slam_amd import _lib
    fn()                                                    # warm-up
    torch.cuda.synchronize()
    out = {k: [] for k in names}
    for _ in range(reps):
        with _lib.kernel_timer(DEV) as kt:
            for _ in range(LAUNCHES):
                fn()
            torch.cuda.synchronize()
        t = kt.read()
        for k in names:
            out[k].append(t[k][0] / LAUNCHES)
    return {k: statistics.median(v) for k, v in out.items()}


def sixteen(planes):
    """Sixteen planes: the found ones and copies of them turned a little, so that every one has samples to reduce."""
    import numpy as np
    out = []
    for i in range(16):
        p = planes[i % len(planes)]
        n = p["normal"] + 0.01 * (i // len(planes)) * np.array([0.3, -0.5, 0.8])
        out.append([*(n / np.linalg.norm(n)), p["offset"]])
    return np.array(out, np.float64)


def bench(n, reps):
    import numpy as np
    import torch
    from go_slam_amd import _lib
    from go_slam_amd import tsdf_planes as TP
    L = _lib.lib()
    vol, up = scene(n)
    planes = vol.find_planes()
    args = TP.find_arguments("tsdf_planes_bench", vol.voxel)
    read_ms = 8.0 * n ** 3 / HBM_COPY_RATE * 1e3
    out = {"lattice": [n] * 3, "voxel_m": vol.voxel, "planes_found": len(planes),
           "inliers": [p["count"] for p in planes], "ms_plain_read_of_tsdf_and_weight": read_ms, "kernels": []}
    if not planes:
        return out
    lat = [_lib.ptr(vol.tsdf), _lib.ptr(vol.weight), *vol.dims]
    fr = [float(vol.lo[0]), float(vol.lo[1]), float(vol.lo[2]), vol.voxel]
    ref = TP.box_centre32(vol.dims, vol.lo, vol.voxel)

    def record(name, ms, **more):
        out["kernels"].append(dict(kernel=name, ms=ms, over_plain_read=ms / read_ms, **more))
        print(json.dumps(out["kernels"][-1]), flush=True)

    votes = torch.zeros((6, 16, 16), dtype=torch.int32, device=DEV)

    def call_votes():
        _lib.check(L.gs_tsdf_plane_votes(*lat, 1.0, 16, _lib.ptr(votes), _lib.stream_ptr(DEV)), "tsdf_planes_bench")
    record("tsdf_plane_votes", windows(call_votes, ("tsdf_plane_votes",), reps)["tsdf_plane_votes"], bins=16)

    for P, pl in ((len(planes), np.array([[*p["normal"], p["offset"]] for p in planes])), (16, sixteen(planes))):
        o0, bin_m, n_bins = TP.offset_bins(vol.dims, vol.lo, vol.voxel, pl[:, :3], args["band"])
        n_d, o_d = torch.as_tensor(np.ascontiguousarray(pl[:, :3])).to(DEV), torch.as_tensor(o0).to(DEV)
        hist = torch.zeros((P, n_bins), dtype=torch.int32, device=DEV)

        def call_offsets():
            _lib.check(L.gs_tsdf_plane_offsets(*lat, *fr, 1.0, _lib.ptr(n_d), _lib.ptr(o_d), P, args["cos2"], bin_m, n_bins,
                                               _lib.ptr(hist), _lib.stream_ptr(DEV)), "tsdf_planes_bench")
        record("tsdf_plane_offsets", windows(call_offsets, ("tsdf_plane_offsets",), reps)["tsdf_plane_offsets"],
               directions=P, n_bins=n_bins, launches=-(-P // ((16384 - 64) // n_bins)))
        p_d = torch.as_tensor(np.ascontiguousarray(pl)).to(DEV)
        ws = torch.empty(L.gs_tsdf_plane_workspace_bytes(P, *vol.dims) // 8, dtype=torch.float64, device=DEV)
        rows = torch.empty((P, 16), dtype=torch.float64, device=DEV)

        def call_moments():
            _lib.check(L.gs_tsdf_plane_moments(*lat, *fr, 1.0, _lib.ptr(p_d), P, args["cos2"], args["band"], float(ref[0]),
                                               float(ref[1]), float(ref[2]), _lib.ptr(ws), _lib.ptr(rows),
                                               _lib.stream_ptr(DEV)), "tsdf_planes_bench")
        t = windows(call_moments, ("tsdf_plane_moments", "tsdf_plane_sum"), reps)
        record("tsdf_plane_moments", t["tsdf_plane_moments"], planes=P, gathers_of_the_lattice=-(-P // 4))
        record("tsdf_plane_sum", t["tsdf_plane_sum"], planes=P, chunks=-(-(n - 1) ** 3 // int(L.gs_tsdf_align_chunk())),
               workspace_bytes=int(ws.numel() * 8))

    for name, fn in (("find_planes", lambda: vol.find_planes()), ("upright", lambda: vol.upright(up_hint=up, heading="walls"))):
        fn()                                                                    # warm-up
        wall = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn()
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
        out[f"ms_{name}_wall"] = statistics.median(wall)
        out[f"{name}_over_plain_read"] = out[f"ms_{name}_wall"] / read_ms
        if name == "upright":
            out["upright_lattice"] = list(res[0].dims)
        del res
        print(json.dumps({k: v for k, v in out.items() if k != "kernels"}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsdf_planes.json"))
    a = ap.parse_args()
    import torch
    from go_slam_amd import _lib
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "launches_per_window": LAUNCHES,
           "chunk": int(_lib.lib().gs_tsdf_align_chunk()), "hbm_copy_bytes_per_s": HBM_COPY_RATE, "sizes": []}
    for n in a.n:
        out["sizes"].append(bench(n, a.reps))
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
