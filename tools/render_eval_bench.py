"""What the rendering evaluation costs per frame, on a randomly initialised map:
    python tools/render_eval_bench.py [--runs 20] [--out profiles/render_eval.json]
Per frame size (480 x 640 and 680 x 1200), each a HIP-event median over --runs after warm-up:
  quality_ms   gs_image_quality (render_eval.image_quality: both launches, workspace and output allocation included);
  torch_ms     the same numbers by plain torch on the same GPU: fp64 conv2d with the same 11 x 11 window over the five
               moment images, then the index and the means (what one would write without the kernel);
  render_ms    Renderer.render_img of the frame (Replica sampling: 24 + 48 samples, perturb 1, ray batches of 5000);
  quality_share = quality_ms / (render_ms + quality_ms).
The tool claims no target: the rendering dominates, and the file records by how much."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def torch_route(pred, gt, pd, gd, w2):
    """pred, gt [H,W,3] fp32; the same outputs by ATen ops, moments in fp64"""
    x = pred.permute(2, 0, 1)[:, None].double()
    y = gt.permute(2, 0, 1)[:, None].double()
    k = w2[None, None]
    mx, my = torch.nn.functional.conv2d(x, k), torch.nn.functional.conv2d(y, k)
    vx = torch.nn.functional.conv2d(x * x, k) - mx * mx
    vy = torch.nn.functional.conv2d(y * y, k) - my * my
    cov = torch.nn.functional.conv2d(x * y, k) - mx * my
    c1, c2 = 0.01 * 0.01, 0.03 * 0.03
    s = ((2 * mx * my + c1) * (2 * cov + c2)) / ((mx * mx + my * my + c1) * (vx + vy + c2))
    mse = ((x - y) ** 2).mean()
    valid = gd > 0
    l1 = (pd.double() - gd.double()).abs()[valid].mean()
    return torch.stack([mse, -10 * torch.log10(mse), s.mean(), l1])


def timed(fn, runs, warmup=3):
    out = None
    for _ in range(warmup):
        out = fn()
    ms = []
    for _ in range(runs):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), ms, out


def measure(H, W, runs, dev):
    import go_slam_amd.neus as N
    from go_slam_amd.neus import render_eval as RE
    torch.manual_seed(3)
    model = N.InstantNeuS({}, [[-4.0, 4.0]] * 3, device=str(dev)).to(dev)
    R = N.Renderer(N_samples=24, N_surface=48, perturb=1.0, ray_batch_size=5000, points_batch_size=10000, H=H, W=W,
                   fx=0.9 * W, fy=0.9 * W, cx=W / 2 - 0.5, cy=H / 2 - 0.5)
    c2w = torch.eye(4, device=dev)
    gd = torch.rand(H, W, device=dev) * 3.5 + 0.5
    gd[torch.rand(H, W, device=dev) < 0.1] = 0.0
    gt = torch.rand(H, W, 3, device=dev)
    out = R.render_img(model, c2w, dev, gt_depth=gd)
    pred, pd = out["color"].reshape(H, W, 3), out["depth"].reshape(H, W)
    g = torch.from_numpy(RE.gaussian_window()).to(dev)
    w2 = g[:, None] * g[None, :]
    q_ms, q_all, q = timed(lambda: RE.image_quality(pred, gt, pd, gd), runs)
    t_ms, t_all, t = timed(lambda: torch_route(pred, gt, pd, gd, w2), runs)
    r_ms, r_all, _ = timed(lambda: R.render_img(model, c2w, dev, gt_depth=gd), max(3, runs // 4), warmup=2)
    q, t = q.cpu(), t.cpu()
    return {"H": H, "W": W, "runs": runs, "quality_ms": q_ms, "torch_ms": t_ms, "render_ms": r_ms,
            "quality_share": q_ms / (r_ms + q_ms), "torch_over_quality": t_ms / q_ms,
            "outputs": dict(zip(RE.QUALITY_KEYS[:6], q[:6].tolist())),
            "torch_minus_kernel": [float(t[i] - q[i]) for i in range(4)],
            "quality_ms_all": [round(v, 4) for v in q_all], "torch_ms_all": [round(v, 4) for v in t_all],
            "render_ms_all": [round(v, 4) for v in r_all]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="480x640,680x1200")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_eval.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = [measure(*map(int, s.split("x")), a.runs, dev) for s in a.sizes.split(",")]
    for r in res:
        print(json.dumps({k: v for k, v in r.items() if not k.endswith("_all")}))
    data = {"device": torch.cuda.get_device_name(0), "sampling": "24+48, perturb 1, B 5000, points_batch_size 1e4",
            "timing": "HIP events around one call, median of --runs after warm-up, device idle otherwise",
            "results": res}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(data, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
