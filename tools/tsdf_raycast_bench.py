"""TSDF raycast on one GPU, written to profiles/tsdf_raycast.json:
    timeout -k 10 600 python tools/tsdf_raycast_bench.py [--reps 5] [--n 256] [--out profiles/tsdf_raycast.json]
A room-sized lattice (n^3 points over 8 m, synth's wall and floor fused from 16 frames of its arc at 480 x 640 with
colour) is raycast from those 16 poses at 480 x 640 with colour, step 0.5 voxels:
  the kernel's own time (library kernel timer) with the brick flags and without them, and the brick-flag launch;
  whether the two sets of images are equal;
  the share of samples the flags skip, counted by the serial restatement (tests/tsdf_raycast_restatement.py) on the host
  for every eighth pixel of the first pose."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from go_slam_amd import _lib, synth                                # noqa: E402
from go_slam_amd.tsdf import TSDFVolume, c2w_matrices             # noqa: E402
import tsdf_raycast_restatement as RR                              # noqa: E402

DEV = "cuda:0"
H, W = 480, 640
INTR = (577.590698, 578.729797, 318.905426, 242.683609)
K = 16
STEP = 0.5


def kernel_ms(fn, name, reps):
    out = []
    for _ in range(reps):
        with _lib.kernel_timer(DEV) as kt:
            fn()
            torch.cuda.synchronize()
        out.append(kt.read()[name][0])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsdf_raycast.json"))
    a = ap.parse_args()
    n = a.n
    voxel, lo = 8.0 / n, (-4.0, -4.0, -2.0)
    vol = TSDFVolume([[l, l + (n - 1) * voxel] for l in lo], voxel, device=DEV)
    assert vol.dims == (n, n, n), vol.dims
    poses = synth.arc_poses(K).to(DEV)
    disp = synth.plane_disps(poses, torch.tensor(INTR, device=DEV), H, W)
    depth = torch.where(disp > 0, 1.0 / disp, torch.zeros_like(disp)).contiguous()
    vol.integrate(depth, poses, INTR, images=torch.rand(K, 3, H, W, device=DEV))

    def flags_only():
        vol._flags = None
        vol.brick_flags()

    skipped = vol.raycast(poses, INTR, (H, W), step=STEP)          # warm-up of both paths
    plain = vol.raycast(poses, INTR, (H, W), step=STEP, skip=False)
    same = all(torch.equal(skipped[k].view(torch.int32), plain[k].view(torch.int32)) for k in skipped)
    t_skip = kernel_ms(lambda: vol.raycast(poses, INTR, (H, W), step=STEP), "tsdf_raycast", a.reps)
    t_plain = kernel_ms(lambda: vol.raycast(poses, INTR, (H, W), step=STEP, skip=False), "tsdf_raycast", a.reps)
    t_flags = kernel_ms(flags_only, "tsdf_brick_flags", a.reps)
    flags = vol.brick_flags().cpu().numpy()

    host = {"tsdf": vol.tsdf.cpu().numpy(), "weight": vol.weight.cpu().numpy()}
    coarse = (INTR[0] / 8, INTR[1] / 8, (INTR[2] + 0.5) / 8 - 0.5, (INTR[3] + 0.5) / 8 - 0.5)
    stats = {}
    RR.raycast(host, c2w_matrices(poses[:1].cpu()).numpy(), coarse, (H // 8, W // 8), lo, voxel, step=STEP, color=False,
               flags=flags, stats=stats)
    out = {
        "device": torch.cuda.get_device_name(0), "reps": a.reps, "lattice": [n, n, n], "voxel": voxel, "frames": K,
        "image": [H, W], "step_voxels": STEP,
        "ms_raycast_kernel_with_flags": statistics.median(t_skip), "ms_raycast_kernel_with_flags_all": t_skip,
        "ms_raycast_kernel_without_flags": statistics.median(t_plain), "ms_raycast_kernel_without_flags_all": t_plain,
        "ms_brick_flags_kernel": statistics.median(t_flags), "ms_brick_flags_kernel_all": t_flags,
        "with_and_without_flags_equal_bits": same,
        "hit_share": float((skipped["depth"] > 0).float().mean()),
        "bricks_flagged": int(flags.sum()), "bricks": int(flags.size),
        "samples_counted_on_host": stats["samples"],
        "share_of_samples_skipped": 1.0 - stats["evaluated"] / max(stats["samples"], 1),
    }
    print(json.dumps({k: v for k, v in out.items() if not k.endswith("_all")}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
