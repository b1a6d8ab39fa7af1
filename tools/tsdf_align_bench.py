"""SDF pose alignment on one GPU, written to profiles/tsdf_align.json:
    python tools/tsdf_align_bench.py --build-variants          (no GPU: the three chunk sizes, each a library of its own)
    timeout -k 10 900 python tools/tsdf_align_bench.py [--reps 5] [--n 256] [--out profiles/tsdf_align.json]
A room-sized lattice (n^3 points over 8 m, synth's wall and floor fused from 16 frames of its arc at 480 x 640) and the
depth maps of that arc:
  the kernels' own time (library kernel timer) of one gs_tsdf_align_system -- the gather and the chunk sum -- at strides
  4, 2 and 1 for 1, 8 and 64 poses, and the bytes it asks for (4 of depth and 64 of corners per sampled pixel) over
  that time against the 8 TB/s of HBM: a figure for a gather, whose cells are shared by neighbouring pixels and
  mostly come from the caches;
  the same for one pose at strides 4 and 1 and for 8 and 64 poses at stride 1 for libgoslam_hip_align_<chunk>.so,
  chunk 1024, 2048 and 4096, each in a process of its own (a library is loaded once per process) and each between two
  runs of the shipped library (A B A B A B A);
  the wall time of one `align` with the default levels and of `relocalize` over 512 candidates.
Medians of --reps."""
import argparse
import glob
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CSRC = os.path.join(ROOT, "go_slam_amd", "csrc")
CHUNKS = (1024, 2048, 4096)
DEV = "cuda:0"
H, W = 480, 640
INTR = (577.590698, 578.729797, 318.905426, 242.683609)
K = 16
LAUNCHES = 10                    # per timed window
HBM_PEAK = 8.0e12
VARIANT_CASES = ((1, 4), (1, 1), (8, 1), (64, 1))          # (poses, stride) measured per chunk size


def variant_path(chunk):
    return os.path.join(CSRC, f"libgoslam_hip_align_{chunk}.so")


def build_variants():
    """libgoslam_hip_align_<chunk>.so = the shipped library's objects with tsdf_align.hip compiled at that chunk size
    (the Makefile's flags)."""
    from go_slam_amd import _lib
    _lib.build()
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wall", "-Wno-unused-function",
             "-fno-gpu-rdc", "-munsafe-fp-atomics"]
    objs = sorted(o for o in glob.glob(os.path.join(CSRC, "*.o")) if os.path.basename(o) != "tsdf_align.o")
    for c in CHUNKS:
        obj = os.path.join(CSRC, f"tsdf_align.o.{c}")
        subprocess.run([hipcc] + flags + [f"-DTSDF_ALIGN_CHUNK={c}", "-c", os.path.join(CSRC, "tsdf_align.hip"), "-o", obj],
                       check=True)
        subprocess.run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", variant_path(c)] + objs + [obj], check=True)
        print("built", variant_path(c))


def scene(n):
    import torch
    from go_slam_amd import synth
    from go_slam_amd.tsdf import TSDFVolume
    voxel, lo = 8.0 / n, (-4.0, -4.0, -2.0)
    vol = TSDFVolume([[l, l + (n - 1) * voxel] for l in lo], voxel, device=DEV)
    assert vol.dims == (n, n, n), vol.dims
    poses = synth.arc_poses(K).to(DEV)
    disp = synth.plane_disps(poses, torch.tensor(INTR, device=DEV), H, W)
    depth = torch.where(disp > 0, 1.0 / disp, torch.zeros_like(disp)).contiguous()
    vol.integrate(depth, poses, INTR)
    from go_slam_amd.lietorch_shim import SE3
    c2w = SE3(poses.double()).inv().matrix().cpu().numpy()
    return vol, depth, c2w


def system_ms(vol, depth, c2w, B, stride, reps):
    """Median kernel time [ms] of one system call (gather, chunk sum) for B poses spread over the K maps."""
    import numpy as np
    import torch
    from go_slam_amd import _lib, localize
    frame = (np.arange(B) % K).astype(np.int32)
    s = localize._Systems(vol, depth, frame, list(INTR), 0.5, float("inf"), 1.0, "tsdf_align_bench")
    bufs = localize._buffers(vol.device, np.ascontiguousarray(c2w[frame, :3, :]), s.workspace_bytes(B, stride))
    s.system(stride, *bufs)                                 # warm-up
    torch.cuda.synchronize()
    gather, total = [], []
    for _ in range(reps):
        with _lib.kernel_timer(DEV) as kt:
            for _ in range(LAUNCHES):
                s.system(stride, *bufs)
            torch.cuda.synchronize()
        t = kt.read()
        gather.append(t["tsdf_align_system"][0] / LAUNCHES)
        total.append((t["tsdf_align_system"][0] + t["tsdf_align_sum"][0]) / LAUNCHES)
    rows = bufs[1].cpu().numpy()
    return statistics.median(gather), statistics.median(total), float(rows[:, 28].mean())


def one(n, reps):
    """What a child process measures for the library it loaded: VARIANT_CASES."""
    from go_slam_amd import _lib
    vol, depth, c2w = scene(n)
    out = {"chunk": int(_lib.lib().gs_tsdf_align_chunk())}
    for B, stride in VARIANT_CASES:
        g, t, count = system_ms(vol, depth, c2w, B, stride, reps)
        out[f"ms_gather_b{B}_s{stride}"], out[f"ms_system_b{B}_s{stride}"] = g, t
    return out


def child(lib_path, n, reps):
    env = dict(os.environ)
    if lib_path:
        env["GOSLAM_HIP_LIB"] = lib_path
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", "--n", str(n), "--reps", str(reps)], env=env,
                         stdout=subprocess.PIPE, text=True, timeout=300, check=True)
    return json.loads(res.stdout.strip().splitlines()[-1])


def wall_ms(fn, reps):
    import torch
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsdf_align.json"))
    ap.add_argument("--build-variants", action="store_true")
    ap.add_argument("--one", action="store_true")
    a = ap.parse_args()
    if a.build_variants:
        build_variants()
        return
    if a.one:
        print(json.dumps(one(a.n, a.reps)), flush=True)
        return
    import numpy as np
    import torch
    from go_slam_amd import _lib, localize
    vol, depth, c2w = scene(a.n)
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "launches_per_window": LAUNCHES,
           "lattice": [a.n] * 3, "image": [H, W], "chunk": int(_lib.lib().gs_tsdf_align_chunk()), "system": []}
    for stride in (4, 2, 1):
        samples = -(-H // stride) * -(-W // stride)
        for B in (1, 8, 64):
            g, t, count = system_ms(vol, depth, c2w, B, stride, a.reps)
            asked = B * samples * 68
            out["system"].append({"stride": stride, "poses": B, "samples_per_pose": samples, "mean_count": count,
                                  "ms_gather": g, "ms_system": t, "bytes_asked": asked,
                                  "asked_bytes_per_s": asked / (g * 1e-3), "share_of_hbm_peak": asked / (g * 1e-3) / HBM_PEAK})
            print(json.dumps(out["system"][-1]), flush=True)

    rng = np.random.default_rng(0)
    start = c2w[:1].copy()
    start[0, :3, 3] += [0.0, 0.02, 0.03]
    vol.align(depth[:1], start, INTR)                                           # warm-up
    out["ms_align_default_levels_one_pose"] = wall_ms(lambda: vol.align(depth[:1], start, INTR), a.reps)
    centres = np.stack([c2w[0, :3, 3] + rng.normal(size=3) * [1.0, 0.1, 1.0] for _ in range(64)])
    cand = localize.candidate_poses(centres, 8, 1, up_sign=-1)
    found = localize.relocalize(vol, depth[0], INTR, cand)
    out["relocalize_candidates"] = int(cand.shape[0])
    out["relocalize_found"] = bool(found["found"])
    out["ms_relocalize_512_candidates"] = wall_ms(lambda: localize.relocalize(vol, depth[0], INTR, cand), a.reps)

    out["chunk_variants"] = []
    missing = [c for c in CHUNKS if not os.path.exists(variant_path(c))]
    if missing:
        out["chunk_variants_missing"] = missing
    else:
        for c in CHUNKS:                                                        # A B A B A B, closed by a last A
            out["chunk_variants"].append(dict(child(None, a.n, a.reps), library="shipped"))
            out["chunk_variants"].append(dict(child(variant_path(c), a.n, a.reps), library=f"align_{c}"))
            print(json.dumps(out["chunk_variants"][-2:]), flush=True)
        out["chunk_variants"].append(dict(child(None, a.n, a.reps), library="shipped"))
    print(json.dumps({k: v for k, v in out.items() if k not in ("system", "chunk_variants")}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
