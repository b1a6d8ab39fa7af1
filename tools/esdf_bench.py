"""Distance field of the TSDF volume on one GPU, written to profiles/esdf.json:
    timeout -k 10 600 python tools/esdf_bench.py [--reps 5] [--n 256] [--out profiles/esdf.json]
The room-sized lattice of tools/tsdf_raycast_bench.py (n^3 points over 8 m, synth's wall and floor fused from 16 frames
of its arc at 480 x 640).  For max_distance 1 m and None (unbounded):
  the kernels' own times (library kernel timer) of the build, per pass, of a query of 1 M points and of a slice;
  the wall time of scipy.ndimage.distance_transform_edt over the same site mask on the host, and whether its squared
  distances, under the same band rule, equal the kernels' d2.
Nothing here is a comparison of like with like: the host transform is one thread of another algorithm.  The numbers are
recorded, no ratio is claimed."""
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
from go_slam_amd import _lib, synth                                # noqa: E402
from go_slam_amd.tsdf import TSDFVolume                            # noqa: E402

DEV = "cuda:0"
H, W = 480, 640
INTR = (577.590698, 578.729797, 318.905426, 242.683609)
K = 16
FAR = 0x7fffffff
BUILD = ("esdf_sites_z", "esdf_pass_y", "esdf_pass_x", "esdf_finish")


def kernel_ms(fn, names, reps):
    """{name: [ms per repetition]} of the named launches inside fn."""
    out = {name: [] for name in names}
    for _ in range(reps):
        with _lib.kernel_timer(DEV) as kt:
            fn()
            torch.cuda.synchronize()
        got = kt.read()
        for name in names:
            out[name].append(got[name][0])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "esdf.json"))
    a = ap.parse_args()
    n = a.n
    voxel, lo = 8.0 / n, (-4.0, -4.0, -2.0)
    vol = TSDFVolume([[l, l + (n - 1) * voxel] for l in lo], voxel, device=DEV)
    assert vol.dims == (n, n, n), vol.dims
    poses = synth.arc_poses(K).to(DEV)
    disp = synth.plane_disps(poses, torch.tensor(INTR, device=DEV), H, W)
    depth = torch.where(disp > 0, 1.0 / disp, torch.zeros_like(disp)).contiguous()
    vol.integrate(depth, poses, INTR)
    g = torch.Generator(device=DEV).manual_seed(3)
    points = torch.rand(1 << 20, 3, generator=g, device=DEV) * ((n - 1) * voxel) + torch.tensor(lo, device=DEV)

    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "lattice": [n, n, n], "voxel": voxel, "frames": K,
           "query_points": int(points.shape[0]), "fields": {}}
    site = None
    for max_distance in (1.0, None):
        field = vol.esdf(max_distance)                             # warm-up
        field.query(points)
        field.occupancy_slice(1, (-0.5, 0.5), robot_radius=0.25)
        t_build = kernel_ms(lambda: vol.esdf(max_distance), BUILD, a.reps)
        t_query = kernel_ms(lambda: field.query(points), ("esdf_query",), a.reps)
        t_slice = kernel_ms(lambda: field.occupancy_slice(1, (-0.5, 0.5), robot_radius=0.25), ("esdf_slice",), a.reps)
        d2 = field.d2.cpu().numpy()
        state = field.state.cpu().numpy()
        if site is None:
            from scipy.ndimage import distance_transform_edt
            site = d2 == 0
            t0 = time.perf_counter()
            edt = distance_transform_edt(~site)
            t_host = time.perf_counter() - t0
            exact = np.rint(edt ** 2).astype(np.int64)
        R = field.radius_voxels
        same = bool(np.array_equal(np.where(exact > R * R, FAR, exact), d2)) if site.any() else bool((d2 == FAR).all())
        rec = {"radius_voxels": R, "d2_equals_host_edt": same,
               "ms_build_kernels": sum(statistics.median(t_build[k]) for k in BUILD),
               "ms_query_kernel": statistics.median(t_query["esdf_query"]),
               "ms_slice_kernel": statistics.median(t_slice["esdf_slice"]),
               "share_far": float((d2 == FAR).mean())}
        for k in BUILD:
            rec[f"ms_{k}_kernel"] = statistics.median(t_build[k])
            rec[f"ms_{k}_kernel_all"] = t_build[k]
        rec["ms_query_kernel_all"], rec["ms_slice_kernel_all"] = t_query["esdf_query"], t_slice["esdf_slice"]
        out["fields"]["none" if max_distance is None else repr(max_distance)] = rec
        out.update(sites=int(site.sum()), share_unknown=float((state == 0).mean()), share_solid=float((state == 2).mean()))
    out["s_host_scipy_edt_wall"] = t_host
    print(json.dumps({k: ({f: {m: v for m, v in r.items() if not m.endswith("_all")} for f, r in val.items()}
                          if k == "fields" else val) for k, val in out.items()}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
