"""How well the neural map reproduces the frames it was trained on, at the end of a run: PSNR, SSIM and depth L1 of
`Renderer.render_img` against the input frames (no counterpart in the reference, whose src/image_visualization.py stops
at a per-frame MAE / PSNR over the pixels with depth while it draws a figure).

`image_quality` is one call of gs_image_quality (csrc/image_quality.hip; contract in include/goslam_neus.h): the whole
image, valid 11 x 11 Gaussian windows, no clipping, fp64 moments.  `eval_rendering` runs it over every `every`-th frame
of a sequence with the poses `SLAM.terminate` evaluates and meshes with, keeps the per-frame results on the device and
reads them once.  tests/image_quality_restatement.py restates the kernel on the CPU.
"""
import ctypes
import os

import numpy as np
import torch

from .. import _lib

QUALITY_KEYS = ("mse", "psnr", "ssim", "depth_l1", "n_depth", "n_windows", "reserved0", "reserved1")
WINDOW = 11                                   # taps of the Gaussian window; H, W >= WINDOW
SIGMA = 1.5
REPORT_ORDER = ("psnr", "ssim", "depth_l1_cm", "n_frames")     # order of the lines of metrics_render.txt


def gaussian_window():
    """The normalised 1-D weights g_k = exp(-(k-5)^2 / 4.5) / sum as fp64 [11]; the 2-D window is their outer product."""
    k = np.arange(WINDOW, dtype=np.float64) - (WINDOW - 1) / 2
    e = np.exp(-(k * k) / (2.0 * SIGMA * SIGMA))
    return e / e.sum()


def tile_shape():
    """(rows, columns) of window positions one workgroup of the kernel owns (GS_IQ_TILE_H, GS_IQ_TILE_W)."""
    th, tw = ctypes.c_int(0), ctypes.c_int(0)
    _lib.check(_lib.lib().gs_image_quality_tile(ctypes.byref(th), ctypes.byref(tw)), "gs_image_quality_tile")
    return th.value, tw.value


def _interleaved(img, name):
    """[H,W,3] as it is; [3,H,W] or [1,3,H,W] (the dataset items) permuted once.  A 3-D shape that reads both ways,
    [3,W,3], is taken as interleaved."""
    if not torch.is_tensor(img):
        raise TypeError(f"image_quality: {name} must be a tensor")
    if img.dim() == 4 and img.shape[0] == 1 and img.shape[1] == 3:
        return img[0].permute(1, 2, 0)
    if img.dim() == 3 and img.shape[2] == 3:
        return img
    if img.dim() == 3 and img.shape[0] == 3:
        return img.permute(1, 2, 0)
    raise ValueError(f"image_quality: {name} must be [H,W,3], [3,H,W] or [1,3,H,W], not {list(img.shape)}")


def image_quality(pred_rgb, gt_rgb, pred_depth=None, gt_depth=None):
    """Device fp64 [8] in QUALITY_KEYS order for one frame.  pred_rgb, gt_rgb: [H,W,3], or planar [3,H,W] / [1,3,H,W];
    pred_depth, gt_depth: H W values each (any shape), both or neither.  Nothing is clipped.  Raises ValueError for
    mismatched shapes, half a depth pair or an image smaller than the window, RuntimeError for CPU tensors."""
    pred, gt = _interleaved(pred_rgb, "pred_rgb"), _interleaved(gt_rgb, "gt_rgb")
    if pred.shape != gt.shape:
        raise ValueError(f"image_quality: pred_rgb {list(pred.shape)} and gt_rgb {list(gt.shape)} differ")
    H, W = int(pred.shape[0]), int(pred.shape[1])
    if H < WINDOW or W < WINDOW:
        raise ValueError(f"image_quality: a {H} x {W} image is smaller than the {WINDOW} x {WINDOW} window")
    if (pred_depth is None) != (gt_depth is None):
        raise ValueError("image_quality: pred_depth and gt_depth are given both or neither")
    if pred_depth is not None and (pred_depth.numel() != H * W or gt_depth.numel() != H * W):
        raise ValueError(f"image_quality: the depth images must have {H} x {W} values")
    tensors = [pred, gt] + ([pred_depth, gt_depth] if pred_depth is not None else [])
    if not all(t.is_cuda for t in tensors):
        raise RuntimeError("image_quality: every input must be a GPU tensor (go_slam_amd has no CPU fallback)")
    dev = pred.device
    pred = pred.detach().to(torch.float32).contiguous()
    gt = gt.detach().to(dev, torch.float32).contiguous()
    pd = gd = None
    if pred_depth is not None:
        pd = pred_depth.detach().to(dev, torch.float32).reshape(H, W).contiguous()
        gd = gt_depth.detach().to(dev, torch.float32).reshape(H, W).contiguous()
    L = _lib.lib()
    nbytes = L.gs_image_quality_workspace_bytes(H, W)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out = torch.empty(8, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        rc = L.gs_image_quality(_lib.ptr(pred), _lib.ptr(gt), _lib.ptr(pd), _lib.ptr(gd), H, W, _lib.ptr(out),
                                _lib.ptr(ws), nbytes, _lib.stream_ptr(dev))
    _lib.check(rc, "gs_image_quality")
    return out


def frame_mean(values):
    """The mean the report uses: the sum in frame order, divided by the count; NaN without a value."""
    total = 0.0
    for v in values:
        total += float(v)
    return total / len(values) if len(values) else float("nan")


def summarize(frames, per_frame):
    """frames: the evaluated indices; per_frame: host fp64 [F,8].  -> the reported dict: the means over frames of psnr
    and ssim, of depth_l1 in cm over the frames that have a depth pixel, and n_frames."""
    rows = np.asarray(per_frame, dtype=np.float64).reshape(len(frames), 8)
    with_depth = [r[3] for r in rows if r[4] > 0]
    return {"psnr": frame_mean(rows[:, 1]), "ssim": frame_mean(rows[:, 2]),
            "depth_l1_cm": 100.0 * frame_mean(with_depth), "n_frames": len(frames)}


def metrics_text(result, frames, per_frame, metric_depth=True):
    """The text of metrics_render.txt: two header lines, `name<TAB>value` per reported value, then one line per
    evaluated frame, `index psnr ssim depth_l1` (depth_l1 in m, as the kernel gives it).  Values are written with repr():
    reading the file gives back the fp64 numbers bit for bit."""
    depth = "depth L1 over the pixels with sensor depth" if metric_depth else \
        "depth L1 is nan: monocular depth has no metric scale"
    lines = ["Rendering of the neural map against the input frames: PSNR (data range 1, whole image, not clipped), "
             "SSIM (11x11 Gaussian window, sigma 1.5, valid windows, per channel)",
             f"(means over the evaluated frames; {depth}; then per frame: index psnr ssim depth_l1[m])"]
    lines += [f"{k}\t{result[k]!r}" for k in REPORT_ORDER]
    rows = np.asarray(per_frame, dtype=np.float64).reshape(len(frames), 8)
    lines += [f"{int(i)} {float(r[1])!r} {float(r[2])!r} {float(r[3])!r}" for i, r in zip(frames, rows)]
    return "\n".join(lines) + "\n"


def parse_metrics(text):
    """metrics_text's inverse: (reported dict, [(index, psnr, ssim, depth_l1), ...])."""
    lines = text.splitlines()
    if len(lines) < 2 + len(REPORT_ORDER) or not lines[0].startswith("Rendering") or "SSIM" not in lines[0]:
        raise ValueError("not a metrics_render.txt")
    result = {}
    for key, line in zip(REPORT_ORDER, lines[2:]):
        name, value = line.split("\t")
        if name != key:
            raise ValueError(f"metrics_render.txt: expected {key}, found {name}")
        result[key] = int(value) if key == "n_frames" else float(value)
    frames = []
    for line in lines[2 + len(REPORT_ORDER):]:
        i, p, s, d = line.split(" ")
        frames.append((int(i), float(p), float(s), float(d)))
    return result, frames


def _save_side_by_side(path, pred, gt):
    """rendered | input, [H,W,3] each, as one JPEG"""
    from PIL import Image
    both = torch.cat([pred, gt.to(pred.device)], dim=1).clamp(0.0, 1.0).mul(255.0).round().to(torch.uint8)
    Image.fromarray(both.cpu().numpy()).save(path, quality=95)


def eval_rendering(slam, stream, c2w_list, every=5, out_path=None, save_images=False):
    """Render every `every`-th frame of `stream` from its pose in `c2w_list` (the map's frame: what terminate holds as
    estimate_c2w_list) and compare it with the input frame.  In rgbd mode the sensor depth guides the sampling, as in
    mapping, and the depth pair is compared; otherwise neither.  The per-frame results stay on the device in one [F,8]
    tensor and are read once.  Returns summarize()'s dict plus `frames` and `per_frame` (host fp64 [F,8]); with
    `out_path` writes that file, with `save_images` also render_eval/{i:05d}.jpg beside it."""
    every = int(every)
    if every < 1:
        raise ValueError("eval_rendering: every must be at least 1")
    if save_images and out_path is None:
        raise ValueError("eval_rendering: save_images needs out_path (the images go beside it)")
    device = slam.mapping_net.bound.device
    rgbd = slam.mode == "rgbd"
    img_dir = None
    if save_images:
        img_dir = os.path.join(os.path.dirname(os.path.abspath(out_path)), "render_eval")
        os.makedirs(img_dir, exist_ok=True)
    frames, rows = [], []
    for i in range(0, len(stream), every):
        _, color, depth, _, _ = stream[i]
        gt_rgb = _interleaved(color, "the stream's colour").to(device, torch.float32)
        H, W = gt_rgb.shape[0], gt_rgb.shape[1]
        gt_depth = depth.to(device, torch.float32) if rgbd else None
        out = slam.renderer.render_img(slam.mapping_net, c2w_list[i], device, gt_depth=gt_depth)
        pred_rgb = out["color"].reshape(H, W, 3)
        rows.append(image_quality(pred_rgb, gt_rgb, out["depth"].reshape(H, W) if rgbd else None, gt_depth))
        frames.append(i)
        if img_dir is not None:
            _save_side_by_side(os.path.join(img_dir, f"{i:05d}.jpg"), pred_rgb, gt_rgb)
    per_frame = (torch.stack(rows) if rows else torch.zeros(0, 8, dtype=torch.float64)).cpu().numpy()   # the one read
    result = summarize(frames, per_frame)
    if out_path is not None:
        with open(out_path, "w") as fh:
            fh.write(metrics_text(result, frames, per_frame, metric_depth=rgbd))
    result.update(frames=frames, per_frame=per_frame)
    return result
