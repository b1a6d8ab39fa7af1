"""TSDF fusion on one GPU, written to profiles/tsdf_fusion.json:
    timeout -k 10 900 python tools/tsdf_bench.py [--reps 5] [--out profiles/tsdf_fusion.json] [--sizes 256 512]
Per lattice size n (n^3 points) and scene, one batch of gs_tsdf_batch() frames at 480 x 640 with colour:
  (a) fused: TSDFVolume.integrate (csrc/tsdf.hip), median wall time and the kernel's own time (library kernel timer);
  (b) torch: the op sequence a user would write today -- per frame, project the whole voxel grid with torch ops, gather
      depth and colour at the rounded pixel, update the running means with torch.where -- on the same inputs;
  and TSDFVolume.extract_mesh of the fused volume.
Scenes: "room" is synth's wall and floor from its arc (8 m lattice: most z-runs are outside every frustum or are skipped
frame by frame); "all_live" puts a 1 m lattice wholly inside every frustum, so every point's state is read and written
once: its 40 bytes per point over the kernel time, as a fraction of the HBM peak, is the kernel's state bandwidth."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from go_slam_amd import _lib, synth                                # noqa: E402
from go_slam_amd.tsdf import TSDFVolume, w2c_matrices              # noqa: E402

HBM_PEAK_GBS = 8000.0
DEV = "cuda:0"
H, W = 480, 640
INTR = (577.590698, 578.729797, 318.905426, 242.683609)
STATE_BYTES_PER_POINT = 2 * 5 * 4          # tsdf, weight and three colour sums, read and written once per batch


def make_frames(k):
    poses = synth.arc_poses(k).to(DEV)
    disp = synth.plane_disps(poses, torch.tensor(INTR, device=DEV), H, W)
    depth = torch.where(disp > 0, 1.0 / disp, torch.zeros_like(disp)).contiguous()
    images = torch.rand(k, 3, H, W, device=DEV)
    return depth, w2c_matrices(poses), images


def make_volume(n, scene):
    if scene == "room":
        voxel, lo = 8.0 / n, (-4.0, -4.0, -2.0)
    else:
        voxel, lo = 1.0 / n, (-0.4, -0.6, 3.4)
    bound = [[l, l + (n - 1.5) * voxel] for l in lo]        # n points: half a voxel short, so rounding cannot add one
    vol = TSDFVolume(bound, voxel, device=DEV)
    assert vol.dims == (n, n, n), vol.dims
    return vol


def torch_integrate(vol, depth, mats, images):
    """The plain-torch sequence: one pass over the whole grid per frame."""
    nx, ny, nz = vol.dims
    fx, fy, cx, cy = INTR
    lo = [float(v) for v in vol.lo]
    px = (lo[0] + torch.arange(nx, device=DEV, dtype=torch.float32) * vol.voxel)[:, None, None]
    py = (lo[1] + torch.arange(ny, device=DEV, dtype=torch.float32) * vol.voxel)[None, :, None]
    pz = (lo[2] + torch.arange(nz, device=DEV, dtype=torch.float32) * vol.voxel)[None, None, :]
    tsdf, weight, colors = vol.tsdf, vol.weight, vol.colors
    for f, m in enumerate(mats.cpu().tolist()):
        z = ((m[2][0] * px + m[2][1] * py) + m[2][2] * pz) + m[2][3]
        x = ((m[0][0] * px + m[0][1] * py) + m[0][2] * pz) + m[0][3]
        y = ((m[1][0] * px + m[1][1] * py) + m[1][2] * pz) + m[1][3]
        fu = torch.floor(fx * (x / z) + cx + 0.5)
        fv = torch.floor(fy * (y / z) + cy + 0.5)
        ok = (z > 1e-3) & (fu >= 0) & (fu < W) & (fv >= 0) & (fv < H)
        pix = fv.clamp(0, H - 1).long() * W + fu.clamp(0, W - 1).long()
        d = depth[f].reshape(-1)[pix]
        sdf = d - z
        ok &= (d > 0) & (sdf >= -vol.trunc)
        s = (sdf / vol.trunc).clamp(max=1.0)
        w1 = weight + 1.0
        tsdf = torch.where(ok, (tsdf * weight + s) / w1, tsdf)
        okc = ok & (sdf <= vol.trunc)
        colors = torch.stack([torch.where(okc, (colors[c] * weight + images[f, c].reshape(-1)[pix]) / w1, colors[c])
                              for c in range(3)])
        weight = torch.where(ok, w1.clamp(max=vol.max_weight), weight)
    return tsdf, weight, colors


def wall_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def run_case(n, scene, frames, reps):
    depth, mats, images = frames
    vol = make_volume(n, scene)
    fused = lambda: vol.integrate(depth, mats, INTR, images=images)      # noqa: E731
    fused()                                                              # warm-up
    t_fused, t_torch = [], []
    for r in range(reps):
        vol.reset()
        t_fused.append(wall_ms(fused)[0])
    vol.reset()
    with _lib.kernel_timer(DEV) as kt:
        fused()
        torch.cuda.synchronize()
    kernel_ms = kt.read()["tsdf_integrate"][0]
    ref = make_volume(n, scene)
    out = None
    for r in range(max(2, reps // 2)):
        del out
        ms, out = wall_ms(lambda: torch_integrate(ref, depth, mats, images))
        t_torch.append(ms)
    touched = float((vol.weight > 0).float().mean())
    same_weight = float((out[1] == vol.weight).float().mean())
    max_diff = float((out[0] - vol.tsdf).abs().max())
    del out, ref
    t_mesh, mesh = [], None
    for r in range(3):
        ms, mesh = wall_ms(vol.extract_mesh)
        t_mesh.append(ms)
    npoints = n ** 3
    res = {
        "lattice": [n, n, n], "voxel": vol.voxel, "frames": int(depth.shape[0]), "image": [H, W],
        "share_of_points_updated": touched,
        "ms_fused_batch": statistics.median(t_fused), "ms_fused_batch_all": t_fused, "ms_fused_kernel": kernel_ms,
        "ms_torch_batch": statistics.median(t_torch), "ms_torch_batch_all": t_torch,
        "torch_over_fused": statistics.median(t_torch) / statistics.median(t_fused),
        "torch_vs_fused_equal_weight_share": same_weight, "torch_vs_fused_max_abs_tsdf_diff": max_diff,
        "ms_extract_mesh": statistics.median(t_mesh), "mesh_vertices": len(mesh.vertices), "mesh_faces": len(mesh.faces),
        "state_bytes_all_points": npoints * STATE_BYTES_PER_POINT,
        "state_gbs_all_points": npoints * STATE_BYTES_PER_POINT / (kernel_ms * 1e-3) / 1e9,
    }
    res["state_fraction_of_hbm_peak"] = res["state_gbs_all_points"] / HBM_PEAK_GBS
    print(scene, n, json.dumps({k: v for k, v in res.items() if not k.endswith("_all")}), flush=True)
    del vol
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsdf_fusion.json"))
    a = ap.parse_args()
    k = int(_lib.lib().gs_tsdf_batch())
    frames = make_frames(k)
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "batch": k, "hbm_peak_gbs": HBM_PEAK_GBS,
           "note": "state_*_all_points counts 40 B for every lattice point; only in the all_live scene is every point's "
                   "state really moved, so only there is state_fraction_of_hbm_peak a bandwidth", "cases": {}}
    for n in a.sizes:
        for scene in ("room", "all_live"):
            out["cases"][f"{scene}_{n}"] = run_case(n, scene, frames, a.reps)
            with open(a.out, "w") as fh:
                json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
