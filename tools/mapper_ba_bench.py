#!/usr/bin/env python
"""Cost of mapping.BA's ray gradients on the fused mapper step -> profiles/mapper_ba.json.

    python tools/mapper_ba_bench.py [--iters 20]

Per batch size (4096, 32768 rays): the BA-off step as the mapper runs it (graph replay), the same step run eagerly, and
the eager ray-gradient step (MapTrainer.step_ray_grad) -- wall time per step after warm-up -- plus the per-kernel split of
one ray-gradient step (library launch timer: gs_neus_backward_raygrad's point pass and ray sums, the pose reduction)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def _problem(n, dev, seed=0):
    from oracle import neus_oracle as O
    import go_slam_amd.neus as N
    P = O.make_params(seed, grid_init=0.05, bound=((-2.5, 2.5), (-2.5, 2.5), (-2.5, 2.5)))
    g = torch.Generator().manual_seed(seed + 1)
    o = (torch.rand(n, 3, generator=g) * 4 - 2).to(dev)
    d = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=1).to(dev)
    gt = (torch.rand(n, generator=g) * 3.5 + 0.5).to(dev)
    col = torch.rand(n, 3, generator=g).to(dev)
    model = N.InstantNeuS({}, P["bound"].tolist()).to(dev)
    with torch.no_grad():
        model.sdf_network.encoding.encoding.params.copy_(P["grid"])
        model.sdf_network.sdf_layer.weight.copy_(P["sdf_w"])
        model.color_network.network.params.copy_(P["mlp"])
        model.color_network._B.copy_(P["color_B"])
    return model, (o, d, col, gt)


def _time(fn, iters, dev):
    for _ in range(3):
        fn()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mapper_ba.json"))
    a = ap.parse_args()
    import go_slam_amd.neus as N
    from go_slam_amd import _lib
    from go_slam_amd.neus.mapper import MapTrainer
    from go_slam_amd.neus.pose import pose_gradients
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(dev), "iters": a.iters, "sizes": {}}
    for n in (4096, 32768):
        R = N.Renderer(N_samples=24, N_surface=48)
        model, args = _problem(n, dev)
        tg = MapTrainer(model, R)                   # (a trainer binds its model's parameters: one model each)
        model_e, _ = _problem(n, dev)
        te = MapTrainer(model_e, R, graph=False)
        row = {"step_graph_ms": _time(lambda: tg.step(*args), a.iters, dev),
               "step_eager_ms": _time(lambda: te.step(*args), a.iters, dev),
               "step_ray_grad_eager_ms": _time(lambda: te.step_ray_grad(*args), a.iters, dev)}
        seg = torch.tensor([0] + [n * (k + 1) // 22 for k in range(22)], dtype=torch.int32, device=dev)
        _, d_rays = te.step_ray_grad(*args)
        dirs = args[1].contiguous()
        row["pose_reduce_ms"] = _time(lambda: pose_gradients(d_rays, dirs, seg), a.iters, dev)
        torch.cuda.synchronize(dev)
        with _lib.kernel_timer(dev) as kt:
            te.step_ray_grad(*args)
            pose_gradients(d_rays, dirs, seg)
            torch.cuda.synchronize(dev)
        row["kernels_ms"] = {k: round(v[0], 4) for k, v in sorted(kt.read().items(), key=lambda kv: -kv[1][0])}
        row["ray_grad_overhead_ms"] = row["step_ray_grad_eager_ms"] - row["step_eager_ms"]
        res["sizes"][str(n)] = row
        print(n, json.dumps(row))
        del tg, te, model, model_e
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
