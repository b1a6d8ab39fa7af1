"""Renderer.render_img against the reference's batch loop, on a randomly initialised map:
    python tools/render_img_bench.py [--runs 10] [--out profiles/render_img.json]
    python tools/render_img_bench.py --only b --runs 1 --sizes 480x640      # one path, for a rocprofv3 --kernel-trace run
    python tools/render_img_bench.py --merge-trace <kernel_trace.csv> --path b --size 480x640 --runs 1
Replica sampling (24 + 48 samples, perturb 1, ray_batch_size 5000, points_batch_size 1e4).  Two paths, alternated in one
process, each timed device-synchronised per image (median of --runs after warm-up):
  (a) the reference's render_img: build_all_rays in torch, then per ray batch render_batch_ray (one gs_render_sample and
      the InstantNeuS forward) and torch.cat of every output;
  (b) Renderer.render_img: gs_render_img_sample (rays, per-batch maxima, samples) and a few segmented forwards.
Also the sampling launch alone (gs_render_img_sample) and its bytes over time.  --merge-trace adds launches per image and
per-kernel times from a rocprofv3 kernel trace (SQLite or CSV) of a --only run to the JSON."""
import argparse
import collections
import csv
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

HBM_PEAK_GBS = 8000.0


def setup(H, W, dev):
    from go_slam_amd import neus as N
    from oracle import neus_oracle as NO
    P = NO.make_params(251, grid_init=0.3, bound=((-4.0, 4.0), (-4.0, 4.0), (-4.0, 4.0)))
    model = N.InstantNeuS({}, P["bound"].tolist()).to(dev)
    with torch.no_grad():
        model.sdf_network.encoding.encoding.params.copy_(P["grid"])
        model.sdf_network.sdf_layer.weight.copy_(P["sdf_w"])
        model.sdf_network.sdf_layer.bias.copy_(P["sdf_b"])
        model.color_network._B.copy_(P["color_B"])
        model.color_network.network.params.copy_(P["mlp"])
    g = torch.Generator().manual_seed(7)
    c2w = torch.eye(4)
    c2w[:3, :3] = torch.linalg.qr(torch.randn(3, 3, generator=g))[0]
    c2w[:3, 3] = torch.randn(3, generator=g) * 0.3
    depth = (torch.rand(H, W, generator=g) * 3.5 + 0.5).to(dev)
    R = N.Renderer(N_samples=24, N_surface=48, perturb=1.0, ray_batch_size=5000, points_batch_size=10000, H=H, W=W,
                   fx=0.9 * W, fy=0.9 * W, cx=W / 2 - 0.5, cy=H / 2 - 0.5)
    return R, model, c2w.to(dev), depth


def path_a(R, model, c2w, depth, dev):
    """the reference's render_img (render.py:177-236) over this package's render_batch_ray"""
    with torch.no_grad():
        H, W = R.H, R.W
        x, y = torch.meshgrid(torch.linspace(0, W - 1, W, device=dev), torch.linspace(0, H - 1, H, device=dev),
                              indexing="ij")
        x, y = x.t(), y.t()
        dirs = torch.stack([(x - R.cx) / R.fx, (y - R.cy) / R.fy, torch.ones_like(x)], dim=-1)
        rays_d = (dirs @ c2w[:3, :3].t()).reshape(-1, 3)
        rays_o = c2w[:3, 3].reshape(1, 1, 3).repeat(H, W, 1).reshape(-1, 3)
        gt = depth.reshape(-1)
        out = {}
        for i in range(0, H * W, R.ray_batch_size):
            o = R.render_batch_ray(rays_o[i:i + R.ray_batch_size], rays_d[i:i + R.ray_batch_size], model, device=dev,
                                   gt_depth=gt[i:i + R.ray_batch_size])
            for k, v in o.items():
                out[k] = torch.cat([out[k], v], dim=0) if k in out else v
        return out


def path_b(R, model, c2w, depth, dev):
    return R.render_img(model, c2w, dev, gt_depth=depth)


def timed(fn, *a):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn(*a)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def measure(H, W, runs, only, dev):
    R, model, c2w, depth = setup(H, W, dev)
    paths = {"a": path_a, "b": path_b}
    if only:
        paths = {only: paths[only]}
    for fn in paths.values():          # warm-up: library load, workspaces, caches
        fn(R, model, c2w, depth, dev)
        fn(R, model, c2w, depth, dev)
    ms = collections.defaultdict(list)
    for _ in range(runs):
        for k, fn in paths.items():
            ms[k].append(timed(fn, R, model, c2w, depth, dev))
    res = {"H": H, "W": W, "rays": H * W, "points": H * W * 72, "runs": runs}
    for k in paths:
        res[f"{k}_ms_median"] = statistics.median(ms[k])
        res[f"{k}_ms_all"] = [round(v, 4) for v in ms[k]]
    if not only:
        res["speedup_a_over_b"] = res["a_ms_median"] / res["b_ms_median"]
        rows = torch.rand(-(-H * W // R.ray_batch_size), 24, device=dev)
        t = []
        for i in range(runs + 2):
            v = timed(R.image_samples, c2w, model.bound, dev, depth, rows)
            if i >= 2:
                t.append(v)
        byt = H * W * (4 + 12 + 12 + 2 * 72 * 4)          # depth read; rays_o, rays_d, z_vals, dists written
        res["sample_ms_median_incl_host"] = statistics.median(t)
        res["sample_bytes"] = byt
    return res


def merge_trace(path, trace, size, runs, tag):
    data = json.load(open(path)) if os.path.exists(path) else {}
    if trace.endswith(".db"):           # rocprofv3's default SQLite output
        import sqlite3
        rows = sqlite3.connect(trace).execute("select name, start, end from kernels").fetchall()
    else:                               # --output-format csv
        rows = [(r["Kernel_Name"], r["Start_Timestamp"], r["End_Timestamp"]) for r in csv.DictReader(open(trace))]
    per = collections.defaultdict(lambda: [0, 0.0])
    for n, t0, t1 in rows:
        n = n.split("(")[0] if n.startswith("_Z") else n[:120]      # (template instances of one kernel stay apart)
        per[n][0] += 1
        per[n][1] += (int(t1) - int(t0)) / 1e3
    images = runs + 2                                   # the measured runs plus the two warm-up images (--only: one path)
    # (the map's setup -- parameter copies, the depth image -- is in the trace as well: a few launches over all images)
    ent = data.setdefault("kernel_trace", {}).setdefault(size, {})
    ent[f"launches_per_image_{tag}"] = sum(v[0] for v in per.values()) / images
    ent[f"kernels_{tag}"] = {
        n: {"launches_per_image": round(c / images, 2), "us_per_image": round(us / images, 2)}
        for n, (c, us) in sorted(per.items(), key=lambda kv: -kv[1][1])[:15]}
    json.dump(data, open(path, "w"), indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="480x640,680x1200")
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--only", choices=["a", "b"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_img.json"))
    ap.add_argument("--merge-trace")
    ap.add_argument("--path", default="b")
    ap.add_argument("--size", default="480x640")
    a = ap.parse_args()
    if a.merge_trace:
        merge_trace(a.out, a.merge_trace, a.size, a.runs, a.path)
        return
    dev = torch.device("cuda:0")
    res = [measure(*map(int, s.split("x")), a.runs, a.only, dev) for s in a.sizes.split(",")]
    for r in res:
        print(json.dumps({k: v for k, v in r.items() if not k.endswith("_all")}))
    if not a.only:
        data = json.load(open(a.out)) if os.path.exists(a.out) else {}
        data.update(device=torch.cuda.get_device_name(0), sampling="24+48, perturb 1, B 5000, points_batch_size 1e4",
                    results=res)
        json.dump(data, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
