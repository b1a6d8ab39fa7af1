"""Volume-to-volume registration and merge on one GPU, written to profiles/tsdf_merge.json:
    timeout -k 10 600 python tools/tsdf_merge_bench.py [--reps 5] [--n 256] [--out profiles/tsdf_merge.json]
Two room-sized volumes (n^3 points over 8 m each): D fused from 16 frames of synth's arc over its wall and floor at 480 x
640, S from the next 16 frames of the arc in a world of its own, 3 cm and 1.5 degrees off D's.
  The kernels' own time (library kernel timer) of one gs_tsdf_register_system -- the gather and the chunk sum -- at
  strides 4, 2 and 1 for 1 and 8 transforms, and the bytes it asks for (8 of S and 64 of D's corners per sample) over
  that time against the 8 TB/s of HBM: a figure for a gather, whose cells are shared by neighbouring samples and mostly
  come from the caches.
  One gs_tsdf_merge of S into a copy of D with colours, the bytes it asks for (32 of S's weights per point whose image
  has a cell in S, 128 more of tsdf and colours where that cell was seen, 40 of D read and written per fused point) and
  what a streaming pass over D alone (20 bytes read and 20 written per point) would take at HBM's peak.
  Beside it the one yardstick in the tree that moves comparable bytes: one gs_tsdf_integrate launch of one frame with
  colours on D's lattice.
  The wall time of one `register` with the default levels.
No parent commit registers or merges volumes: there is no ratio against one.  Medians of --reps windows of 10 launches."""
import argparse
import json
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
HBM_PEAK = 8.0e12


def s_to_d():
    """S-world to D-world, float64 [3,4]: 3 cm and 1.5 degrees about fixed directions."""
    import math

    import numpy as np
    w = np.array([0.36, -0.48, 0.8]) * math.radians(1.5)
    th = float(np.linalg.norm(w))
    Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    R = np.eye(3) + math.sin(th) / th * Kx + (1 - math.cos(th)) / th ** 2 * (Kx @ Kx)
    return np.concatenate([R, 0.03 * np.array([[0.6], [0.0], [-0.8]])], 1)


def scene(n):
    import numpy as np
    import torch
    from go_slam_amd import synth
    from go_slam_amd.tsdf import TSDFVolume, w2c_matrices
    voxel, lo = 8.0 / n, (-4.0, -4.0, -2.0)
    poses = synth.arc_poses(2 * K).to(DEV)
    disp = synth.plane_disps(poses, torch.tensor(INTR, device=DEV), H, W)
    depth = torch.where(disp > 0, 1.0 / disp, torch.zeros_like(disp)).contiguous()
    g = torch.Generator(device=DEV).manual_seed(0)
    images = torch.rand(2 * K, 3, H, W, device=DEV, generator=g)
    w2c = w2c_matrices(poses)
    T = np.eye(4)
    T[:3, :] = s_to_d()
    w2c_s = torch.from_numpy(np.stack([(np.vstack([m, [0, 0, 0, 1.0]]) @ T)[:3, :] for m in w2c.double().cpu().numpy()]))
    vols = []
    for sl, mats in ((slice(0, K), w2c), (slice(K, 2 * K), w2c_s)):
        vol = TSDFVolume([[l, l + (n - 1) * voxel] for l in lo], voxel, device=DEV)
        assert vol.dims == (n, n, n), vol.dims
        vol.integrate(depth[sl], mats[sl], INTR, images=images[sl])
        vols.append(vol)
    return vols[0], vols[1], T, (depth[:1].contiguous(), w2c[:1].contiguous(), images[:1].contiguous())


def lattice_args(vol):
    return [*vol.dims, float(vol.lo[0]), float(vol.lo[1]), float(vol.lo[2]), vol.voxel, vol.trunc]


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


def system_ms(D, S, T, B, stride, reps):
    import numpy as np
    import torch
    from go_slam_amd import _lib
    L = _lib.lib()
    pose = torch.from_numpy(np.ascontiguousarray(np.tile(T[:3, :], (B, 1, 1)))).to(DEV)
    rows = torch.empty(B, 32, dtype=torch.float64, device=DEV)
    ws = torch.empty(max(L.gs_tsdf_register_workspace_bytes(B, *S.dims, stride) // 8, 1), dtype=torch.float64, device=DEV)

    def call():
        rc = L.gs_tsdf_register_system(_lib.ptr(D.tsdf), _lib.ptr(D.weight), *lattice_args(D), _lib.ptr(S.tsdf),
                                       _lib.ptr(S.weight), *lattice_args(S), _lib.ptr(pose), B, stride, 1.0, 0.5, _lib.ptr(ws),
                                       _lib.ptr(rows), _lib.stream_ptr(DEV))
        _lib.check(rc, "tsdf_merge_bench")
    t = windows(call, ("tsdf_register_system", "tsdf_register_sum"), reps)
    r = rows.cpu().numpy()
    return t["tsdf_register_system"], t["tsdf_register_system"] + t["tsdf_register_sum"], float(r[:, 28].mean()), float(r[:, 30].mean())


def merge_counts(D, S, T, before, after):
    """(points of D whose image has a cell in S, those whose cell was seen at all eight corners, those fused): the first
    two from the contract's geometry restated with torch in fp32 (a count for a bandwidth figure, not a test), the third
    from the weights before and after."""
    import numpy as np
    import torch
    from go_slam_amd.tsdf_merge import inverse32
    m = torch.from_numpy(inverse32(T[:3, :])).to(DEV)
    ax = [torch.tensor(float(D.lo[a]), device=DEV) + torch.arange(D.dims[a], device=DEV, dtype=torch.float32) * D.voxel
          for a in range(3)]
    inside = None
    cells = []
    for r in range(3):
        ps = ((m[r, 0] * ax[0][:, None, None] + m[r, 1] * ax[1][None, :, None]) + m[r, 2] * ax[2][None, None, :]) + m[r, 3]
        a = torch.floor((ps - float(S.lo[r])) / S.voxel)
        ok = (a >= 0) & (a < S.dims[r] - 1)
        inside = ok if inside is None else inside & ok
        cells.append(a.clamp(0, S.dims[r] - 2).long())
    seen = inside.clone()
    for i in (0, 1):
        for j in (0, 1):
            for k in (0, 1):
                seen &= S.weight[cells[0] + i, cells[1] + j, cells[2] + k] >= 1.0
    return int(inside.sum()), int(seen.sum()), int((before != after).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsdf_merge.json"))
    a = ap.parse_args()
    import torch
    from go_slam_amd import _lib
    D, S, T, frame = scene(a.n)
    npoints = a.n ** 3
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "launches_per_window": LAUNCHES, "lattice": [a.n] * 3,
           "voxel_m": 8.0 / a.n, "chunk": int(_lib.lib().gs_tsdf_align_chunk()), "system": []}
    for stride in (4, 2, 1):
        samples = (-(-a.n // stride)) ** 3
        for B in (1, 8):
            g, t, count, considered = system_ms(D, S, T, B, stride, a.reps)
            asked = B * samples * 72
            out["system"].append({"stride": stride, "transforms": B, "samples_per_transform": samples, "mean_count": count,
                                  "mean_considered": considered, "ms_gather": g, "ms_system": t, "bytes_asked": asked,
                                  "asked_bytes_per_s": asked / (g * 1e-3), "share_of_hbm_peak": asked / (g * 1e-3) / HBM_PEAK})
            print(json.dumps(out["system"][-1]), flush=True)

    # the merge: D is restored afterwards; the weights reach their cap after a few launches, which changes no work
    tsdf0, weight0, colors0 = D.tsdf.clone(), D.weight.clone(), D.colors.clone()
    D.merge(S, T)
    counts = merge_counts(D, S, T, weight0, D.weight)
    D.tsdf.copy_(tsdf0), D.weight.copy_(weight0), D.colors.copy_(colors0)
    ms_merge = windows(lambda: D.merge(S, T), ("tsdf_merge",), a.reps)["tsdf_merge"]
    D.tsdf.copy_(tsdf0), D.weight.copy_(weight0), D.colors.copy_(colors0)
    inside, seen, fused = counts
    asked = inside * 32 + seen * 128 + fused * 40
    stream = npoints * 40
    out["merge"] = {"points": npoints, "points_with_a_source_cell": inside, "points_with_a_seen_cell": seen,
                    "points_fused": fused, "ms_merge": ms_merge, "bytes_asked": asked,
                    "asked_bytes_per_s": asked / (ms_merge * 1e-3), "share_of_hbm_peak": asked / (ms_merge * 1e-3) / HBM_PEAK,
                    "bytes_streaming_pass_over_d": stream, "ms_streaming_pass_at_hbm_peak": stream / HBM_PEAK * 1e3}
    print(json.dumps(out["merge"]), flush=True)

    depth, w2c, images = frame
    ms_int = windows(lambda: D.integrate(depth, w2c, INTR, images=images), ("tsdf_integrate",), a.reps)["tsdf_integrate"]
    D.tsdf.copy_(tsdf0), D.weight.copy_(weight0), D.colors.copy_(colors0)
    out["integrate_one_frame"] = {"ms_integrate": ms_int, "merge_over_integrate": ms_merge / ms_int}
    print(json.dumps(out["integrate_one_frame"]), flush=True)

    D.register(S, T)                                                            # warm-up
    wall = []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = D.register(S, T)
        wall.append((time.perf_counter() - t0) * 1e3)
    out["ms_register_default_levels_one_transform"] = statistics.median(wall)
    out["register_ok"] = bool(res["ok"][0])
    out["register_overlap"] = float(res["overlap"][0])
    print(json.dumps({k: v for k, v in out.items() if k not in ("system", "merge", "integrate_one_frame")}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
