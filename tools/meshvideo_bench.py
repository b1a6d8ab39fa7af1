"""Mesh-video timings on one GPU, written to profiles/meshvideo.json:
    python tools/meshvideo_bench.py [--res 512] [--reps 20] [--out profiles/meshvideo.json]

The mesh is the marching-cubes mesh tools/mesh_bench.py extracts (same network, bound and resolution), coloured; the frame
is 1080 x 1920 with MeshVideo's default intrinsics, seen from outside the room; the overlay is 200 camera actors and two
1000-point trajectories.  Per frame, median ms by HIP events after warm-up:
  visbuf (gs_mesh_visbuf, incl. its buffer fill), gs_mesh_depth on the same mesh, pose and camera in the same run (the
  yardstick: the same work with 32-bit atomics and half the buffer), lines (gs_line_visbuf), resolve (gs_visbuf_resolve,
  also as achieved bytes/s: 8 B read + 3 B written per pixel, plus per covered pixel three vertex gathers of
  12 + 3 + 12 B and 12 B of face indices), the vertex normals once per mesh, and a whole MeshVideo tick with the JPEG
  write (host clock around a call that ends in the device-to-host copy)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from go_slam_amd import _lib, meshvideo as MV    # noqa: E402
import go_slam_amd.neus as N                     # noqa: E402
from go_slam_amd.neus.mesher import render_mesh_depth  # noqa: E402
from oracle import neus_oracle as O              # noqa: E402
from tools.mesh_bench import timed               # noqa: E402

HBM_COPY_RATE = 6.29e12
H, W = 1080, 1920


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "meshvideo.json"))
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
    model.update_bound(torch.tensor([[-1.6, 1.7], [-1.2, 2.2], [-0.7, 2.6]]))
    m = model.extract_geometry(args.res, 0.0, save_path=None, color=True)
    fx, fy, cx, cy = MV.default_intrinsics(H, W)
    # the viewer: outside the room, looking at its centre
    eye, target = np.array([6.5, -3.0, 4.5]), np.array([0.0, 0.5, 1.0])
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross(z, [0.0, 0.0, 1.0])
    x /= np.linalg.norm(x)
    view = np.eye(4)
    view[:3, 0], view[:3, 1], view[:3, 2], view[:3, 3] = x, np.cross(z, x), z, eye
    g = np.random.default_rng(0)
    t = np.linspace(0, 4 * np.pi, 1000)
    traj = np.stack([1.2 * np.cos(t), 0.5 + 1.2 * np.sin(t), 1.0 + 0.3 * np.sin(3 * t)], 1)
    c2w = np.tile(np.eye(4), (1000, 1, 1))
    c2w[:, :3, 3] = traj
    gt = c2w.copy()
    gt[:, :3, 3] += g.normal(size=(1000, 3)) * 0.01

    mesh = MV.upload_mesh(m, dev)
    w2c = MV.world_to_camera(torch.from_numpy(view[None]), dev)
    rec = {"device": torch.cuda.get_device_name(0), "frame": [H, W], "resolution": args.res,
           "vertices": int(mesh.vertices.shape[0]), "faces": int(mesh.faces.shape[0]), "reps": args.reps,
           "statistic": "median ms per frame, HIP events, after 2 warm-up calls", "hbm_copy_rate_Bps": HBM_COPY_RATE}
    with tempfile.TemporaryDirectory() as tmp:
        init = view.copy()                      # MeshVideo's viewer ends at `view` (viewer_extrinsic)
        init[:3, 1:3] *= -1
        init[:3, 3] = view[:3, 3] - 2 * init[:3, 2]
        video = MV.MeshVideo(tmp, init, cam_scale=0.08, save_rendering=True, estimate_c2w_list=c2w, gt_c2w_list=gt,
                             device=dev).start()
        video.mesh = mesh
        for i in range(0, 1000, 10):
            video.render = i == 990             # only the last message of the build-up draws
            video.update_pose(i, c2w[i].copy(), is_keyframe=True)
            video.update_pose(i, gt[i].copy(), is_gt=True, is_keyframe=True)
        video.render = False
        video.update_cam_trajectory(1000, False)
        video.render = True
        video.update_cam_trajectory(1000, True)
        segs_np, cols_np = video.scene()
        segs = torch.from_numpy(segs_np).to(dev, torch.float32)
        cols = torch.from_numpy(np.rint(cols_np * 255)).to(dev, torch.uint8)
        rec["segments"] = int(segs.shape[0])

        L, st = _lib.lib(), _lib.stream_ptr(dev)
        ws = torch.empty(L.gs_mesh_visbuf_workspace_bytes(), dtype=torch.uint8, device=dev)
        vb = torch.empty(1, H, W, dtype=torch.int64, device=dev)
        img = torch.empty(1, H, W, 3, dtype=torch.uint8, device=dev)
        depth = torch.empty(1, H, W, dtype=torch.float32, device=dev)
        cam = (fx, fy, cx, cy, H, W, MV.ZNEAR, MV.ZFAR)
        V, F = mesh.vertices.shape[0], mesh.faces.shape[0]

        def visbuf():
            _lib.check(L.gs_mesh_visbuf(_lib.ptr(mesh.vertices), V, _lib.ptr(mesh.faces), F, _lib.ptr(w2c), 1, *cam,
                                        _lib.ptr(vb), _lib.ptr(ws), ws.numel(), st), "mesh_visbuf")

        def depth_map():
            _lib.check(L.gs_mesh_depth(_lib.ptr(mesh.vertices), V, _lib.ptr(mesh.faces), F, _lib.ptr(w2c), 1, *cam,
                                       _lib.ptr(depth), _lib.ptr(ws), ws.numel(), st), "mesh_depth")

        def lines():
            _lib.check(L.gs_line_visbuf(_lib.ptr(segs), segs.shape[0], F, _lib.ptr(w2c), 1, *cam, _lib.ptr(vb), st),
                       "line_visbuf")

        def resolve():
            MV.resolve_visbuf(vb, mesh, w2c, fx, fy, cx, cy, cols, out=img)

        # the two rasterisers alternate, so that whatever else the machine does touches both alike
        pairs = [(timed(visbuf, 3, warmup=1), timed(depth_map, 3, warmup=1)) for _ in range(max(args.reps // 3, 2))]
        rec["visbuf_ms"] = statistics.median(p[0] for p in pairs)
        rec["mesh_depth_ms"] = statistics.median(p[1] for p in pairs)
        rec["visbuf_over_mesh_depth"] = rec["visbuf_ms"] / rec["mesh_depth_ms"]
        visbuf()
        rec["lines_ms"] = timed(lines, args.reps)
        rec["resolve_ms"] = timed(resolve, args.reps)
        covered = int(((vb != -1) & ((vb & 0xffffffff) < F)).sum())
        rec["covered_pixels"], rec["line_pixels"] = covered, int(((vb != -1) & ((vb & 0xffffffff) >= F)).sum())
        rec["resolve_bytes"] = H * W * 11 + covered * (12 + 3 * (12 + 3 + 12))
        rec["resolve_GBps"] = rec["resolve_bytes"] / (rec["resolve_ms"] * 1e-3) / 1e9
        rec["resolve_share_of_hbm_copy_rate"] = rec["resolve_GBps"] * 1e9 / HBM_COPY_RATE
        rec["vertex_normals_ms"] = timed(lambda: MV.vertex_normals(mesh.vertices, mesh.faces, dev), args.reps)
        # gs_mesh_depth's map and the buffer's high word, on this mesh too
        depth_map()
        visbuf()
        torch.cuda.synchronize()
        hit = depth[0] > 0
        rec["high_word_equals_mesh_depth"] = bool(torch.equal((vb[0] >> 32)[hit].int(), depth[0].view(torch.int32)[hit])
                                                  and bool((vb[0][~hit] == -1).all()))

        def tick():
            video.update_cam_trajectory(1000, True)

        tick()
        ts = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tick()
            ts.append((time.perf_counter() - t0) * 1e3)
        rec["tick_with_jpeg_ms"] = statistics.median(ts)
        video.save_rendering = False

        def tick_sync():
            tick()
            torch.cuda.synchronize()
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            tick_sync()
            ts.append((time.perf_counter() - t0) * 1e3)
        rec["tick_without_jpeg_ms"] = statistics.median(ts)
    print(json.dumps(rec), flush=True)
    old = json.load(open(args.out)) if os.path.exists(args.out) else {}
    if "tests" in old:
        rec["tests"] = old["tests"]            # the shares tests/test_meshvideo_gpu.py records
    with open(args.out, "w") as fh:
        json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
