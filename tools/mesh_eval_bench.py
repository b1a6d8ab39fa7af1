"""Mesh-evaluation timings on one GPU (go_slam_amd.neus.mesh_eval), written to profiles/mesh_evaluation.json:
    python tools/mesh_eval_bench.py [--res 512 1024] [--reps 5] [--out profiles/mesh_evaluation.json]
Scene: tools/cull_bench.py's analytic room (marching cubes at `res`^3 over a 6 m box).  HIP-event medians after a
warm-up, no profiler:
  NNIndex build (grid) on the room's vertices and on 2e5 surface samples;
  exact NN queries: 2e5 samples x 2e5 samples, and 1.2 M noisy vertices x 1.2 M vertices;
  the far-query fixture: ground-truth samples of the whole room against an estimate that lost a third of it (the
  fraction that falls back to brute force, and the time of that query);
  one radius-limited ICP evaluation (query + moments) and a full align_mesh (30 iterations at most);
  a full eval_mesh at 2e5 samples per mesh;
  scipy cKDTree (workers=16) build and query at the same sizes on the host, as the CPU baseline."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from go_slam_amd.neus.mesh import Mesh                      # noqa: E402
from go_slam_amd.neus import mesh_eval as ME                # noqa: E402
from cull_bench import room                                 # noqa: E402


def timed(fn, reps, warmup=1):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def host_timed(fn, reps):
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ts)


def ckdtree(r, q, reps):
    from scipy.spatial import cKDTree
    build = host_timed(lambda: cKDTree(r), reps)
    tree = cKDTree(r)
    query = host_timed(lambda: tree.query(q, workers=16), reps)
    return {"build_ms": build, "query_ms": query}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_evaluation.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    out = {"device": torch.cuda.get_device_name(dev), "timing": "HIP events, median of reps after one warm-up",
           "cpu_baseline": "scipy.spatial.cKDTree, workers=16, host perf_counter", "runs": []}
    for res in a.res:
        try:
            v, f = room(res, dev)
        except torch.cuda.OutOfMemoryError:
            out["runs"].append({"res": res, "skipped": "out of memory building the room"})
            continue
        mesh = Mesh(v.cpu().numpy(), f.cpu().numpy())
        del v, f
        torch.cuda.empty_cache()
        V = len(mesh.vertices)
        n = min(V, 1_200_000)
        g = np.random.default_rng(0)
        r_big = mesh.vertices[:n]
        q_big = r_big[g.permutation(n)] + g.normal(scale=0.005, size=(n, 3))
        np.random.seed(43)
        s_est = ME.sample_surface(mesh, 200_000)
        s_gt = ME.sample_surface(mesh, 200_000)
        run = {"res": res, "vertices": V, "faces": len(mesh.faces), "big_n": n}
        rb = torch.from_numpy(r_big).to(dev)
        qb = torch.from_numpy(q_big).to(dev)
        se, sg = torch.from_numpy(s_est).to(dev), torch.from_numpy(s_gt).to(dev)
        run["grid_build_ms"] = {"big": timed(lambda: ME.NNIndex(rb, dev), a.reps),
                                "2e5": timed(lambda: ME.NNIndex(se, dev), a.reps)}
        ib, ie = ME.NNIndex(rb, dev), ME.NNIndex(se, dev)
        run["grid"] = {"big": {"h": ib.h, "dims": ib.dims}, "2e5": {"h": ie.h, "dims": ie.dims}}
        run["query_ms"] = {"2e5x2e5": timed(lambda: ie.query(sg), a.reps),
                           "big_x_big": timed(lambda: ib.query(qb), a.reps)}
        ie.query(sg)
        fb_near = int(ie.fallback.item())
        # far-query fixture: the estimate lost every surface with x > 1 (a third of the room); ground truth is whole
        keep = s_est[:, 0] <= 1.0
        ipart = ME.NNIndex(torch.from_numpy(s_est[keep]).to(dev), dev)
        run["far_fixture"] = {"estimate_points": int(keep.sum()), "queries": len(s_gt),
                              "query_ms": timed(lambda: ipart.query(sg), a.reps)}
        ipart.query(sg)
        torch.cuda.synchronize()
        run["far_fixture"]["fallback_queries"] = int(ipart.fallback.item())
        run["far_fixture"]["fallback_fraction"] = run["far_fixture"]["fallback_queries"] / len(s_gt)
        run["query_fallbacks_2e5x2e5"] = fb_near
        # ICP: the source is the room displaced by a few degrees and centimetres
        T_true = np.eye(4)
        c, s = np.cos(np.deg2rad(2.0)), np.sin(np.deg2rad(2.0))
        T_true[:2, :2] = [[c, -s], [s, c]]
        T_true[:3, 3] = [0.03, -0.02, 0.01]
        src = r_big @ np.linalg.inv(T_true)[:3, :3].T + np.linalg.inv(T_true)[:3, 3]
        srcd = torch.from_numpy(src).to(dev)
        run["icp_one_iteration_ms"] = timed(
            lambda: ME.registration_icp(srcd, None, 0.1, max_iteration=0, target_index=ib), a.reps)
        res_icp = ME.registration_icp(srcd, None, 0.1, target_index=ib)
        run["icp"] = {"iterations": res_icp.iterations, "fitness": res_icp.fitness, "inlier_rmse": res_icp.inlier_rmse,
                      "max_abs_T_error": float(np.abs(res_icp.transformation - T_true).max())}
        est_big = Mesh(src, mesh.faces[np.all(mesh.faces < n, axis=1)])
        run["align_mesh_ms"] = timed(lambda: ME.align_mesh(est_big.copy(), Mesh(r_big, est_big.faces)), max(1, a.reps // 2))
        np.random.seed(43)
        run["eval_mesh_ms"] = timed(lambda: ME.eval_mesh(mesh, mesh, N3d=2e5, dist_th=0.05), max(1, a.reps // 2))
        run["ckdtree"] = {"2e5x2e5": ckdtree(s_est, s_gt, 3), "big_x_big": ckdtree(r_big, q_big, 3),
                          "far_fixture": ckdtree(s_est[keep], s_gt, 3)}
        out["runs"].append(run)
        print(json.dumps(run), flush=True)
        del ib, ie, ipart, rb, qb, se, sg, srcd
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
