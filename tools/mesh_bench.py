"""Mesh extraction timings on one GPU (InstantNeuS.extract_geometry and its parts), written to
profiles/mesh_extraction.json:
    python tools/mesh_bench.py [--res 256 512] [--reps 5] [--out profiles/mesh_extraction.json]
A model with a random ('trained-like') hash table (oracle.neus_oracle.make_params) and a realtime bound smaller than the
bound.  Per resolution, HIP-event times after warm-up, median of `reps`:
  extract_fields (as it stands: chunked encode + addmm + select, then the volume to the host), sdf_lattice (the fused
  launch), the marching cubes' count / scan / emit launches (the host read of the totals between scan and emit is not in
  any of the three), marching_cubes as called (incl. that read and the output allocation), extract_geometry end to end
  with and without colour (save_path=None).
Also V / F, the workspace bytes, and the marching cubes' bytes per second: the bytes its three launches must move at
least (u read by count and emit: 8 B per lattice point; the 2-byte point record written and read back: 4 B; vertices and
faces written: 12 B each) over their summed time, against the 6.29 TB/s measured copy rate (MI355X_MICROARCH.md)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from go_slam_amd import _lib                     # noqa: E402
import go_slam_amd.neus as N                     # noqa: E402
from go_slam_amd.neus.mesh import marching_cubes  # noqa: E402
from oracle import neus_oracle as O              # noqa: E402

COPY_RATE = 6.29e12


def timed(fn, reps, warmup=2):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_extraction.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    P = O.make_params(83, grid_init=0.2, bound=((-2.0, 2.0), (-1.5, 2.5), (-1.0, 3.0)))
    model = N.InstantNeuS({}, P["bound"].tolist(), device=dev).to(dev)
    with torch.no_grad():
        model.sdf_network.encoding.encoding.params.copy_(P["grid"])
        model.sdf_network.sdf_layer.weight.copy_(P["sdf_w"])
        model.sdf_network.sdf_layer.bias.copy_(P["sdf_b"] + 0.05)
        model.color_network._B.copy_(P["color_B"])
        model.color_network.network.params.copy_(P["mlp"])
    rt = torch.tensor([[-1.6, 1.7], [-1.2, 2.2], [-0.7, 2.6]])
    model.update_bound(rt)
    L = _lib.lib()
    st = _lib.stream_ptr(dev)
    out = {"device": torch.cuda.get_device_name(0), "bound": P["bound"].tolist(), "realtime_bound": rt.tolist(),
           "reps": args.reps, "statistic": "median ms, HIP events, after 2 warm-up calls", "copy_rate_Bps": COPY_RATE,
           "results": []}
    bmin, bmax = model.bound[:, 0], model.bound[:, 1]
    for r in args.res:
        rec = {"resolution": r, "lattice_points": r ** 3}
        rec["extract_fields_ms"] = timed(lambda: model.extract_fields(bmin, bmax, r), args.reps)
        u = model.sdf_lattice(bmin, bmax, r)
        rec["sdf_lattice_ms"] = timed(lambda: model.sdf_lattice(bmin, bmax, r), args.reps)
        rec["sdf_lattice_inside_fraction"] = float((u != -100.0).float().mean())
        ws_bytes = L.gs_mcubes_workspace_bytes(r, r, r)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        totals = torch.empty(2, dtype=torch.int64, device=dev)

        def count():
            _lib.check(L.gs_mcubes_count(_lib.ptr(u), r, r, r, 0.0, _lib.ptr(ws), ws_bytes, st), "count")

        def scan():
            _lib.check(L.gs_mcubes_scan(r, r, r, _lib.ptr(ws), ws_bytes, _lib.ptr(totals), st), "scan")
        count()
        scan()
        nv, nf = (int(t) for t in totals.cpu())
        verts = torch.empty(nv, 3, dtype=torch.float32, device=dev)
        faces = torch.empty(nf, 3, dtype=torch.int32, device=dev)

        def emit():
            _lib.check(L.gs_mcubes_emit(_lib.ptr(u), r, r, r, 0.0, _lib.ptr(ws), ws_bytes, nv, nf, _lib.ptr(verts),
                                        _lib.ptr(faces), st), "emit")
        # scan rewrites count's workgroup totals in place: the phases are timed as count -> scan -> emit sequences, one
        # event between consecutive launches
        phases = []
        for it in range(2 + args.reps):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            ev[0].record()
            count()
            ev[1].record()
            scan()
            ev[2].record()
            emit()
            ev[3].record()
            torch.cuda.synchronize()
            if it >= 2:
                phases.append([ev[k].elapsed_time(ev[k + 1]) for k in range(3)])
        for k, name in enumerate(("mc_count_ms", "mc_scan_ms", "mc_emit_ms")):
            rec[name] = statistics.median(ph[k] for ph in phases)
        rec["marching_cubes_call_ms"] = timed(lambda: marching_cubes(u, 0.0), args.reps)
        v2, f2 = marching_cubes(u, 0.0)
        assert torch.equal(v2, verts) and torch.equal(f2, faces)
        del v2, f2, ws
        rec.update(vertices=nv, faces=nf, workspace_bytes=ws_bytes)
        mc_ms = rec["mc_count_ms"] + rec["mc_scan_ms"] + rec["mc_emit_ms"]
        mc_bytes = 12 * r ** 3 + 12 * nv + 12 * nf
        rec["mc_min_bytes"] = mc_bytes
        rec["mc_bytes_per_s"] = mc_bytes / (mc_ms * 1e-3)
        rec["mc_fraction_of_copy_rate"] = rec["mc_bytes_per_s"] / COPY_RATE
        del u, verts, faces
        torch.cuda.empty_cache()
        reps_e2e = max(2, args.reps // 2)
        rec["extract_geometry_ms"] = timed(lambda: model.extract_geometry(r, 0.0, save_path=None), reps_e2e, warmup=1)
        rec["extract_geometry_color_ms"] = timed(lambda: model.extract_geometry(r, 0.0, save_path=None, color=True),
                                                 reps_e2e, warmup=1)
        m = model.extract_geometry(r, 0.0, save_path=None)
        rec["mesh_vertices"], rec["mesh_faces"] = len(m.vertices), len(m.faces)
        torch.cuda.empty_cache()
        out["results"].append(rec)
        print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
