"""Dataset frame ingest on one GPU, written to profiles/frame_ingest.json:
    python tools/frame_ingest_bench.py [--frames 300] [--out profiles/frame_ingest.json]
Two sequences are generated from a seed in a temporary directory: TUM layout (640 x 480 colour PNG, 16-bit depth PNG,
the shipped tum.yaml camera: 384 x 512 with 8-pixel edges) and Replica layout (1200 x 680 colour JPEG, 16-bit depth
PNG, replica.yaml: 320 x 640).  Per sequence:
  * device time per frame of each frame_prep kernel (library kernel timer over load_batch calls of 8 frames);
  * bytes uploaded and copied back per frame (the dataset's counters, host output);
  * frames/s of the prefetching iterator (host output) with 1, 4 and 8 decoder threads, and of decoding alone with the
    same pools (the host bound)."""
import argparse
import json
import os
import sys
import tempfile
import time
import types
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from go_slam_amd import _lib, datasets as D          # noqa: E402

DEV = "cuda:0"


def _frame(g, h, w):
    yy, xx = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
    base = np.stack([np.sin(5 * xx + k) * np.cos(4 * yy + 2 * k) for k in range(3)], -1)
    img = np.clip(127.5 + 100 * base + g.normal(0, 6, (h, w, 3)), 0, 255).astype(np.uint8)
    depth = (8000 + 9000 * xx * yy + g.integers(0, 200, (h, w))).astype(np.uint16)
    return img, depth


def write_tum(root, n, g):
    os.makedirs(os.path.join(root, "rgb"))
    os.makedirs(os.path.join(root, "depth"))
    with open(os.path.join(root, "rgb.txt"), "w") as fr, open(os.path.join(root, "depth.txt"), "w") as fd, \
            open(os.path.join(root, "groundtruth.txt"), "w") as fp:
        fp.write("# timestamp tx ty tz qx qy qz qw\n")
        for i in range(n):
            t = 1000.0 + 0.04 * i                          # 25 fps: the 32 fps thinning keeps every frame
            img, depth = _frame(g, 480, 640)
            Image.fromarray(img).save(os.path.join(root, "rgb", f"{t:.6f}.png"))
            Image.fromarray(depth).save(os.path.join(root, "depth", f"{t:.6f}.png"))
            fr.write(f"{t:.6f} rgb/{t:.6f}.png\n")
            fd.write(f"{t:.6f} depth/{t:.6f}.png\n")
            fp.write(f"{t:.4f} {0.01 * i} 0 0 0 0 0 1\n")
    cfg = {"dataset": "tumrgbd", "mode": "rgbd", "stride": 1, "data": {"input_folder": root},
           "cam": {"H": 480, "W": 640, "fx": 517.3, "fy": 516.5, "cx": 318.6, "cy": 255.3, "png_depth_scale": 5000.0,
                   "H_out": 384, "W_out": 512, "H_edge": 8, "W_edge": 8}}
    return cfg


def write_replica(root, n, g):
    os.makedirs(os.path.join(root, "results"))
    with open(os.path.join(root, "traj.txt"), "w") as f:
        for i in range(n):
            img, depth = _frame(g, 680, 1200)
            Image.fromarray(img).save(os.path.join(root, "results", f"frame{i:06d}.jpg"), quality=95)
            Image.fromarray(depth).save(os.path.join(root, "results", f"depth{i:06d}.png"))
            T = np.eye(4)
            T[0, 3] = 0.01 * i
            f.write(" ".join(f"{v:.6f}" for v in T.reshape(-1)) + "\n")
    cfg = {"dataset": "replica", "mode": "rgbd", "stride": 1, "data": {"input_folder": root},
           "cam": {"H": 680, "W": 1200, "fx": 600.0, "fy": 600.0, "cx": 599.5, "cy": 339.5, "png_depth_scale": 6553.5,
                   "H_out": 320, "W_out": 640, "H_edge": 0, "W_edge": 0}}
    return cfg


def measure(cfg, n, batch=8):
    args = types.SimpleNamespace(input_folder=None, max_frames=-1)
    out = {"frames": n}
    # device time per kernel: decoded frames, then batches of `batch` frames through the kernels (device output)
    ds = D.get_dataset(cfg, args, device=DEV, output="device")
    frames = [(i, ds.decode(i)) for i in range(min(n, 64))]
    ds._prep(frames[:batch])                                   # warm-up (maps, allocator)
    torch.cuda.synchronize()
    side = ds._dev_state["stream"]
    with torch.cuda.stream(side):
        with _lib.kernel_timer(DEV) as t:
            for lo in range(0, len(frames), batch):
                ds._prep(frames[lo:lo + batch])
        times = t.read()
    torch.cuda.synchronize()
    nf = len(frames)
    out["kernel_us_per_frame"] = {k: 1e3 * ms / nf for k, (ms, _) in times.items()}
    out["launches_per_batch_of_%d" % batch] = {k: c / ((nf + batch - 1) // batch) for k, (_, c) in times.items()}
    # bytes per frame with the reference's host output
    ds = D.get_dataset(cfg, args, device=DEV)
    ds.load_batch(list(range(batch)))
    out["h2d_bytes_per_frame"] = ds.bytes_h2d / batch
    out["d2h_bytes_per_frame"] = ds.bytes_d2h / batch
    img = D.read_color(ds.color_paths[0])
    out["float32_upload_bytes_per_frame_if_host_preprocessed"] = 4 * 3 * (cfg["cam"]["H_out"] * cfg["cam"]["W_out"]) \
        + 4 * cfg["cam"]["H_out"] * cfg["cam"]["W_out"]
    out["decoded_size"] = list(img.shape)
    for threads in (1, 4, 8):
        ds = D.get_dataset(cfg, args, device=DEV, decode_threads=threads)
        t0 = time.perf_counter()
        k = sum(1 for _ in ds)
        torch.cuda.synchronize()
        out[f"iterator_fps_{threads}_threads"] = k / (time.perf_counter() - t0)
        with ThreadPoolExecutor(max_workers=threads) as pool:
            t0 = time.perf_counter()
            k = sum(1 for _ in pool.map(ds.decode, range(len(ds))))
            out[f"decode_only_fps_{threads}_threads"] = k / (time.perf_counter() - t0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_ingest.json"))
    a = ap.parse_args()
    g = np.random.default_rng(a.seed)
    result = {"device": torch.cuda.get_device_name(0), "seed": a.seed,
              "note": "iterator frames/s include host decoding (PIL) and the device-to-host copy of each item; "
                      "decode_only is the same pool decoding without the GPU; kernel times from the library's "
                      "kernel timer (HIP events around each launch)"}
    with tempfile.TemporaryDirectory() as tmp:
        for name, writer in (("tum_640x480_png", write_tum), ("replica_1200x680_jpg", write_replica)):
            t0 = time.perf_counter()
            cfg = writer(os.path.join(tmp, name), a.frames, g)
            print(f"{name}: wrote {a.frames} frames in {time.perf_counter() - t0:.1f} s", flush=True)
            result[name] = measure(cfg, a.frames)
            print(json.dumps(result[name]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
