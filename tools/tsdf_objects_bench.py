"""Object finding on one GPU, written to profiles/tsdf_objects.json:
    timeout -k 10 900 python tools/tsdf_objects_bench.py [--reps 5] [--n 256 512] [--out profiles/tsdf_objects.json]
Per n, an analytic room (n^3 points over 8 m, truncation 3 voxels, weight 1) in a world tilted by 20 degrees of roll and 10
of pitch: a floor, a wall, two boxes standing on the floor (one turned by 30 degrees) and a floating ball -- the room of
tests/test_tsdf_objects_cpu.py, at the lattice sizes of a real map.
  The kernels' own time (library kernel timer) over one `find_objects` with the floor and the wall as structure: the mark,
  the relaxation's sweeps (all that were enqueued: `plan.sweep_to_fixed_point` sends them in batches, and the sweeps after
  the quiet one find every flag clear), the roots' count and scan, the table's emit and fold and the extents' init and
  fold.  Beside each the time a plain read of the tsdf and weight lattices (8 bytes per point) would take at 6.29 TB/s, the
  rate a float4 copy reaches on this GPU's HBM, and beside the mark the time of gs_tsdf_plane_votes on the same volume:
  the nearest relative among the plane kernels, with the same gather.
  The wall time of one `find_objects`.
No parent commit finds objects: there is no ratio against one.  Medians of --reps runs."""
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
HBM_COPY_RATE = 6.29e12          # bytes per second, measured float4 copy
EXTENT = 8.0
LO = (-3.0, -4.5, -2.0)
SLAB = 16                        # lattice layers whose distances are formed at a time
NAMES = ("tsdf_object_mark", "frontier_relax", "frontier_count", "frontier_scan", "tsdf_object_emit", "tsdf_object_table",
         "tsdf_object_extents_init", "tsdf_object_extents")


def rotation(axis, deg):
    import numpy as np
    a, b = (axis + 1) % 3, (axis + 2) % 3
    R = np.eye(3)
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    R[a, a], R[a, b], R[b, a], R[b, b] = c, -s, s, c
    return R


def tilt():
    """float64 [4,4], the scene's world to the tilted one: 10 degrees about x, then 20 about z, about the box's middle."""
    import numpy as np
    c = np.array(LO) + 0.5 * EXTENT
    M = np.eye(4)
    M[:3, :3] = rotation(2, 20.0) @ rotation(0, 10.0)
    M[:3, 3] = c - M[:3, :3] @ c
    return M


def scene(n):
    """The room as a TSDFVolume, formed slab by slab on the GPU in fp32, and the tilted world's up."""
    import numpy as np
    import torch
    from go_slam_amd.tsdf import TSDFVolume
    voxel = EXTENT / n
    trunc = 3 * voxel
    vol = TSDFVolume([[l, l + (n - 1) * voxel] for l in LO], voxel, device=DEV, trunc=trunc)
    assert vol.dims == (n, n, n), vol.dims
    M = tilt()
    R = torch.tensor(M[:3, :3], dtype=torch.float32, device=DEV)
    t = torch.tensor(M[:3, 3], dtype=torch.float32, device=DEV)
    boxes = [((0.0, 0.8, 1.0), (0.8, 0.8, 0.6), np.eye(3)), ((1.6, 0.7, 2.5), (1.2, 1.0, 0.5), rotation(1, 30.0))]
    ax = [torch.tensor(LO[a], device=DEV) + voxel * torch.arange(n, device=DEV, dtype=torch.float32) for a in range(3)]
    for i0 in range(0, n, SLAB):
        P = torch.stack(torch.meshgrid(ax[0][i0:i0 + SLAB], ax[1], ax[2], indexing="ij"), -1)
        x = (P - t) @ R                                             # M^-1 x
        d = torch.minimum(1.2 - x[..., 1], 4.0 - x[..., 2])
        for centre, size, turn in boxes:
            q = ((x - torch.tensor(centre, device=DEV)) @ torch.tensor(turn, dtype=torch.float32, device=DEV)).abs() \
                - 0.5 * torch.tensor(size, device=DEV)
            d = torch.minimum(d, q.clamp(min=0).norm(dim=-1) + q.max(-1).values.clamp(max=0))
        d = torch.minimum(d, (x - torch.tensor((0.3, 0.2, 3.0), device=DEV)).norm(dim=-1) - 0.35)
        vol.tsdf[i0:i0 + SLAB] = (d / trunc).clamp(-1.0, 1.0)
    vol.weight.fill_(1.0)
    return vol, M[:3, :3] @ np.array([0.0, -1.0, 0.0])


def bench(n, reps):
    import numpy as np
    import torch
    from go_slam_amd import _lib
    from go_slam_amd import tsdf_objects as TO
    from go_slam_amd import tsdf_planes as TP
    L = _lib.lib()
    vol, up = scene(n)
    planes = vol.find_planes()
    floor = TP.floor_plane(planes, up)
    structure, index = TO.structure_planes(planes, floor)
    read_ms = 8.0 * n ** 3 / HBM_COPY_RATE * 1e3
    out = {"lattice": [n] * 3, "voxel_m": vol.voxel, "planes_found": len(planes), "areas_m2": [p["area_m2"] for p in planes],
           "structure": index, "ms_plain_read_of_tsdf_and_weight": read_ms, "kernels": []}

    votes = torch.zeros((6, 16, 16), dtype=torch.int32, device=DEV)
    lat = [_lib.ptr(vol.tsdf), _lib.ptr(vol.weight), *vol.dims]
    times = {k: [] for k in NAMES + ("tsdf_plane_votes",)}
    launches, wall, obj = {}, [], None
    for rep in range(reps + 1):                                 # the first is the warm-up
        torch.cuda.synchronize()
        with _lib.kernel_timer(DEV) as kt:
            t0 = time.perf_counter()
            obj = vol.find_objects(structure)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            _lib.check(L.gs_tsdf_plane_votes(*lat, 1.0, 16, _lib.ptr(votes), _lib.stream_ptr(DEV)), "tsdf_objects_bench")
            torch.cuda.synchronize()
        t = kt.read()
        if rep == 0:
            continue
        wall.append((t1 - t0) * 1e3)
        for k in times:
            times[k].append(t[k][0])
            launches[k] = t[k][1]
    out.update(counts=[int(v) for v in obj.counts.cpu().tolist()], clusters=obj.n_clusters, boxes=len(obj.boxes),
               box_cells=[b["cells"] for b in obj.boxes], box_size_m=[np.round(b["size_m"], 4).tolist() for b in obj.boxes],
               sweeps_to_the_fixed_point=obj.sweeps, ms_find_objects_wall=statistics.median(wall))
    for k in times:                                             # the last entry: the votes, one launch per run
        ms = statistics.median(times[k])
        out["kernels"].append({"kernel": k, "ms": ms, "launches": launches[k], "over_plain_read": ms / read_ms})
        print(json.dumps(out["kernels"][-1]), flush=True)
    print(json.dumps({k: v for k, v in out.items() if k != "kernels"}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsdf_objects.json"))
    a = ap.parse_args()
    import torch
    from go_slam_amd import frontier
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "brick": list(frontier.brick()),
           "hbm_copy_bytes_per_s": HBM_COPY_RATE, "sizes": []}
    for n in a.n:
        out["sizes"].append(bench(n, a.reps))
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
