"""Mesh-culling timings on one GPU (go_slam_amd.neus.mesher), written to profiles/mesh_culling.json:
    python tools/cull_bench.py [--res 512 1024] [--poses 2000] [--reps 3] [--out profiles/mesh_culling.json]
Scene: marching cubes of an analytic room (walls, a table, a pillar, floating specks) at `res`^3 over a 6 m box; poses
inside the room looking around, 240 x 320, fx = fy = 300.  HIP-event medians after warm-up, no profiler:
  render_mesh_depth per pose (chunks of 256 poses) at each resolution, with the large-triangle count;
  point_masks over all poses (given the depth maps);
  face_components (labels + areas) at each resolution;
  OrientedBoundingBox.compute_from_pointcloud over ~40 M points (a noisy room-surface cloud), with the survivor count;
  Mesher.cull_mesh at the first resolution x all poses (ndarray bound, forecast_radius 25), PLY writes included;
  for comparison, the restatement's torch point_masks loop (tests/cull_restatement.py's formulation) on the GPU over
  200 poses, scaled to all poses."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
import types

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from go_slam_amd.neus.mesh import Mesh, marching_cubes       # noqa: E402
from go_slam_amd.neus import mesher as M                    # noqa: E402

H, W, FX, FY, CX, CY = 240, 320, 300.0, 300.0, 159.5, 119.5


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


def room(res, dev):
    x = torch.linspace(-3.0, 3.0, res, device=dev)
    out = torch.empty(res, res, res, device=dev)
    for i in range(res):                       # slab by slab: 1024^3 temporaries would be 4 GB each
        X = x[i]
        Y, Z = torch.meshgrid(x, x, indexing="ij")
        walls = 2.8 - torch.maximum(torch.maximum(X.abs().expand_as(Y), Y.abs()), (Z * 1.3).abs())
        table = torch.maximum(torch.maximum((X - 0.5).abs() - 0.6, (Y + 0.3).abs() - 0.4), (Z + 0.8).abs() - 0.05)
        pillar = torch.hypot(X + 1.2 + 0 * Y, Y - 1.0) - 0.2
        speck = torch.sqrt((X - 0.4) ** 2 + (Y - 1.5) ** 2 + (Z - 1.0) ** 2) - 0.08
        out[i] = -torch.minimum(torch.minimum(walls, table), torch.minimum(pillar, speck))
    v, f = marching_cubes(out, 0.0)
    del out
    return v.double() / (res - 1) * 6.0 - 3.0, f


def poses(n, seed=0):
    g = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        eye = g.uniform(-1.5, 1.5, 3) * [1, 1, 0.5]
        d = g.normal(size=3)
        d /= np.linalg.norm(d)
        z = d
        x = np.cross(z, [0, 0, 1.0])
        x /= np.linalg.norm(x)
        y = np.cross(z, x)
        m = np.eye(4)
        m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = x, y, z, eye
        out.append(m)
    return torch.from_numpy(np.stack(out))


def torch_point_masks(pts, depth, c2w, r):
    """The reference's per-frame torch loop (tests/cull_restatement.py formulation), on the device."""
    dev = pts.device
    n = pts.shape[0]
    seen = torch.zeros(n, dtype=torch.bool, device=dev)
    fc = torch.zeros_like(seen)
    K = torch.tensor([[FX, 0, CX], [0, FY, CY], [0, 0, 1.0]], device=dev)
    homo = torch.cat([pts, torch.ones(n, 1, device=dev)], 1).reshape(-1, 4, 1)
    for i in range(c2w.shape[0]):
        w2c = torch.inverse(c2w[i])
        uv = K @ (w2c @ homo)[:, :3, :]
        z = uv[:, -1:] + 1e-8
        uv = uv[:, :2] / z
        u, v, z = uv[:, 0, 0], uv[:, 1, 0], z[:, 0, 0]
        inf = (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1) & (z > 0)
        ff = (u >= -r) & (u <= W - 1 + r) & (v >= -r) & (v <= H - 1 + r) & (z > 0)
        g = uv.reshape(1, 1, -1, 2).clone()
        g[..., 0] = g[..., 0] / (W - 1) * 2.0 - 1.0
        g[..., 1] = g[..., 1] / (H - 1) * 2.0 - 1.0
        d = F.grid_sample(depth[i].reshape(1, 1, H, W), g, padding_mode="border", align_corners=True).reshape(-1)
        front = torch.where(d > 0, z < d + 0.05, torch.ones_like(seen))
        seen |= inf & front
        fc |= (inf & front) | (ff & front)
    return seen, fc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--poses", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cloud", type=int, default=40_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_culling.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    c2w = poses(args.poses)
    result = {"image": [H, W], "poses": args.poses, "resolutions": {}}
    meshes = {}
    for res in args.res:
        v, f = room(res, dev)
        v32 = v.float().contiguous()
        meshes[res] = (v, f)
        r = {"vertices": int(v.shape[0]), "faces": int(f.shape[0])}
        K = min(256, args.poses)
        part = c2w[:K]
        ms = timed(lambda: M._render(v32, f, part, H, W, FX, FY, CX, CY, 20.0), args.reps)
        r["render_mesh_depth_ms_per_pose"] = ms / K
        r["render_chunk_poses"] = K
        depth = M._render(v32, f, part, H, W, FX, FY, CX, CY, 20.0)
        r["covered_pixel_fraction"] = float((depth > 0).float().mean())
        r["face_components_ms"] = timed(lambda: M.face_components(f, v, dev), args.reps)
        labels, comp_area, total = M.face_components(f, v, dev)
        r["components"] = int((comp_area > 0).sum())
        result["resolutions"][str(res)] = r
        print(res, r, flush=True)
        del depth, labels, comp_area

    res0 = args.res[0]
    v, f = meshes[res0]
    v32 = v.float().contiguous()
    depth_all = M.render_mesh_depth((v32, f), c2w, H, W, FX, FY, CX, CY, device=dev)
    result["point_masks_ms"] = timed(lambda: M.point_masks(v32, depth_all, c2w, H, W, FX, FY, CX, CY, 25.0, device=dev),
                                     args.reps)
    nt = min(200, args.poses)
    c2w_d = c2w[:nt].float().to(dev)
    t_torch = timed(lambda: torch_point_masks(v32, depth_all, c2w_d, 25.0), 1)
    result["torch_point_masks_ms_scaled"] = t_torch * args.poses / nt
    seen, fc = M.point_masks(v32, depth_all, c2w, H, W, FX, FY, CX, CY, 25.0, device=dev)
    ts, tf = torch_point_masks(v32, depth_all, c2w[:nt].float().to(dev), 25.0)
    s_nt, f_nt = M.point_masks(v32, depth_all[:nt], c2w[:nt], H, W, FX, FY, CX, CY, 25.0, device=dev)
    result["point_masks_mismatch_vs_torch_200_poses"] = int((s_nt != ts).sum() + (f_nt != tf).sum())
    del depth_all

    # OBB over a noisy cloud on the room's surface
    idx = torch.randint(0, v32.shape[0], (args.cloud,), device=dev)
    cloud = (v32[idx] + 0.01 * torch.randn(args.cloud, 3, device=dev)).contiguous()
    box = M.OrientedBoundingBox().to(dev)
    result["obb_points"] = args.cloud
    result["obb_ms"] = timed(lambda: box.compute_from_pointcloud(cloud, extend=0.1), args.reps)
    result["obb_survivors"] = box.survivors
    del cloud, idx

    # whole cull_mesh
    with tempfile.TemporaryDirectory() as tmp:
        slam = types.SimpleNamespace(output=tmp, mapping_net=None, video=None, reload_map=0, verbose=False,
                                     H=H, W=W, fx=FX, fy=FY, cx=CX, cy=CY)
        cfg = {"meshing": {"resolution": res0, "level_set": 0.0, "remove_small_geometry_threshold": 0.2,
                           "get_largest_components": False, "eval_rec": False, "n_points_to_eval": 0,
                           "mesh_threshold_to_eval": 0.05, "gt_mesh_path": "", "forecast_radius": 25},
               "mapping": {"device": "cuda:0"}}
        mesher = M.Mesher(cfg, None, slam)
        base = Mesh(v.cpu().numpy(), f.cpu().numpy())
        bound = np.array([[-2.9, 2.9], [-2.9, 2.9], [-2.5, 2.5]])
        times = []
        for _ in range(args.reps):
            m = base.copy()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            cull, fore = mesher.cull_mesh(m, c2w, bound, os.path.join(tmp, "mesh", "final_raw_mesh.ply"))
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        result["cull_mesh_ms"] = statistics.median(times)
        result["cull_mesh_faces_in_out"] = [int(len(base.faces)), int(len(cull.faces)), int(len(fore.faces))]
    print(json.dumps(result, indent=1))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
