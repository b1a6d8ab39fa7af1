"""Visualizer (reference src/image_visualization.py): render a frame of the map with Renderer.render_img, report its
depth MAE / RMSE, colour PSNR and the |sdf| < 0.01 / 0.02 fractions, and save the reference's 2 x 4 figure.

The metrics, the residual images and the camera-frame normals come from one deterministic HIP reduction
(gs_render_img_metrics: fp64 partial sums in a fixed order); the figure's images leave the device in one copy.  The
depth-error colouring stays numpy on the host (it is a per-figure rebinning, not a hot path).  matplotlib is imported
only when a figure is drawn."""
import os

import numpy as np
import torch

from .. import _lib
from ..droid_backends import _workspace
from .pose import quaternion_to_rt

METRIC_KEYS = ("mse", "psnr", "mae", "rmse", "s0.01", "s0.02", "n_valid", "n_sdf")


def image_metrics(render_out, gt_depth, gt_color, c2w):
    """Camera-frame normals R^T n [HW,3], depth residual [HW] and colour residual [HW,3] (zero where gt < 1e-3), and the
    metrics over the pixels with gt > 1e-3 (a depth of exactly 1e-3 is in the residual images but not in the metrics,
    as in the reference): colour MSE over the k x 3 values, PSNR = -10 log10(MSE), depth MAE and RMSE; the fractions of
    |sdf| < 0.01 and < 0.02 over all HW s values.  NaN where no pixel has depth.  Returns (images dict, metrics: device
    fp64 [8] in the order of METRIC_KEYS)."""
    dev = render_out["depth"].device
    f32 = dict(dtype=torch.float32, device=dev)
    n = render_out["depth"].numel()
    s = render_out["sdf"].shape[-1] if render_out["sdf"].dim() > 1 else 1
    if isinstance(c2w, np.ndarray):
        c2w = torch.from_numpy(c2w)
    c2w = c2w.detach().to(dev, torch.float32).reshape(4, 4).contiguous()
    gt_depth = gt_depth.detach().to(dev, torch.float32).reshape(-1).contiguous()
    gt_color = gt_color.detach().to(dev, torch.float32).reshape(-1, 3).contiguous()
    if gt_depth.numel() != n or gt_color.shape[0] != n:
        raise ValueError("gt_depth / gt_color do not match the rendered image")
    flat = {k: render_out[k].detach().float().contiguous() for k in ("color", "depth", "normal", "sdf")}
    imgs = {"normal_cam": torch.empty(n, 3, **f32), "depth_res": torch.empty(n, **f32),
            "color_res": torch.empty(n, 3, **f32)}
    metrics = torch.empty(8, dtype=torch.float64, device=dev)
    L = _lib.lib()
    ws = _workspace(dev, L.gs_render_img_metrics_workspace_bytes() + 256)
    with torch.cuda.device(dev):
        rc = L.gs_render_img_metrics(_lib.ptr(flat["color"]), _lib.ptr(flat["depth"]), _lib.ptr(flat["normal"]),
                                     _lib.ptr(flat["sdf"]), _lib.ptr(gt_depth), _lib.ptr(gt_color), _lib.ptr(c2w), n, s,
                                     _lib.ptr(imgs["normal_cam"]), _lib.ptr(imgs["depth_res"]),
                                     _lib.ptr(imgs["color_res"]), _lib.ptr(metrics), _lib.ptr(ws), ws.numel(),
                                     _lib.stream_ptr(dev))
    _lib.check(rc, "image_metrics")
    return imgs, metrics


def _rebin(err, lo, hi, start, width):
    """Stretch the errors in (lo, hi] linearly onto [start, start + width] (in place)."""
    sel = (err > lo) & (err <= hi)
    if sel.any():
        v = err[sel]
        err[sel] = (v - v.min()) / (v.max() - v.min() + 1e-7) * width + start
    return err


def depth_err_to_colorbar(est, gt=None, with_bar=False, cmap="jet"):
    """The depth-error image of the reference's figure (image_visualization.py:155-197): |est - gt| where gt > 0 (est > 0
    and gt = 0 without a ground truth), mapped piecewise onto the colour map -- errors in (0, 5 cm] to [0, 0.25], (5, 20
    cm] to [0.25, 0.38], (0.2, 0.5] to [0.38, 0.66], (0.5, 1] to [0.66, 0.83], (1, 2] to [0.83, 0.95] and (2, max(5,
    largest)] to [0.95, 1], each band stretched over its own range -- as [H, W, 3] in [0, 1]; with_bar appends the
    colour bar (50 rows) below it."""
    import matplotlib
    est = np.asarray(est)
    if gt is None:
        gt, valid = np.zeros_like(est), est > 0
    else:
        gt = np.asarray(gt)
        valid = gt > 0
    err = np.abs(est - gt) * valid
    h, w = err.shape
    edges = [0, 0.05, 0.2, 0.5, 1.0, 2.0, max(5.0, err.max())]
    stops = [0, 0.25, 0.38, 0.66, 0.83, 0.95, 1]
    for i in range(1, len(edges)):
        err = _rebin(err, edges[i - 1], edges[i], stops[i - 1], stops[i] - stops[i - 1])
    cm = matplotlib.colormaps[cmap]
    img = cm(err)[:, :, :3]
    if not with_bar:
        return img
    import matplotlib.pyplot as plt
    widths = [0, w // 8, w // 8, w // 4, w // 4, w // 8]
    widths.append(w - sum(widths))
    bar = np.concatenate([np.linspace(stops[i - 1], stops[i], widths[i]) for i in range(1, len(widths))])
    bar_img = cm(np.repeat(bar[None, :], 50, axis=0))[:, :, :3]
    plt.xticks(ticks=np.cumsum(widths), labels=[str(f) for f in edges])
    plt.axis("on")
    return np.concatenate((img, bar_img), axis=0)


class Visualizer:
    """src/image_visualization.py:Visualizer with the same constructor and `vis` arguments; `vis` also returns the
    metrics (the reference returns None)."""

    def __init__(self, vis_dir, renderer, device="cuda:0"):
        self.device = device
        self.vis_dir = vis_dir
        self.renderer = renderer
        os.makedirs(f"{vis_dir}", exist_ok=True)

    def vis(self, idx, gt_depth, gt_color, c2w_or_camera_tensor, net):
        """Render frame `idx` from the pose (a [4,4] c2w, or the 7-vector [qw, qx, qy, qz, tx, ty, tz]), print the
        reference's line, write {vis_dir}/{idx:05d}.jpg and return {mse, psnr, mae, rmse, s0.01, s0.02, n_valid,
        n_sdf}."""
        with torch.no_grad():
            H, W = gt_depth.shape[-2:]
            pose = c2w_or_camera_tensor
            if isinstance(pose, np.ndarray):
                pose = torch.from_numpy(pose)
            c2w = quaternion_to_rt(pose.clone().detach().float()) if pose.dim() == 1 else pose
            render_out = self.renderer.render_img(net, c2w, self.device, gt_depth=gt_depth)
            imgs, metrics = image_metrics(render_out, gt_depth, gt_color, c2w)
            dev = render_out["depth"].device
            # every image the figure needs, and the metrics, in one device-to-host copy
            cols = [gt_depth.to(dev).reshape(-1, 1), render_out["depth"].reshape(-1, 1),
                    render_out["depth_variance"].reshape(-1, 1), gt_color.to(dev).reshape(-1, 3),
                    render_out["color"].reshape(-1, 3), imgs["color_res"], imgs["normal_cam"]]
            packed = torch.cat([c.float() for c in cols], dim=1)
            host = torch.cat([packed.reshape(-1).double(), metrics]).cpu().numpy()
            m = dict(zip(METRIC_KEYS, (float(v) for v in host[-8:])))
            img = host[:-8].astype(np.float32).reshape(H, W, 15)
            gt_depth_np, depth_np, uncertainty_np = img[..., 0], img[..., 1], img[..., 2]
            gt_color_np, color_np, color_residual = img[..., 3:6], img[..., 6:9], img[..., 9:12]
            surface_normal = (img[..., 12:15] * 128 + 128).clip(0, 255)
            # (the reference formats Python's builtin `iter` into this line; it is kept so that logs read the same)
            print(f"Idx {idx} Iter {iter}  MAE: {m['mae']:.4f}, PSNR: {m['psnr']:.4f}, "
                  f"S0.01: {m['s0.01']:.4f}, S0.02: {m['s0.02']:.4f}, ")
            self._figure(idx, gt_depth_np, depth_np, uncertainty_np, gt_color_np, color_np, color_residual,
                         surface_normal)
            return m

    def _figure(self, idx, gt_depth_np, depth_np, uncertainty_np, gt_color_np, color_np, color_residual,
                surface_normal):
        import matplotlib
        from matplotlib.figure import Figure          # (an off-screen figure: pyplot's backend is left alone)
        fig = Figure()
        axs = fig.subplots(2, 4)
        fig.tight_layout()
        valid = gt_depth_np[gt_depth_np > 0]
        cmap = matplotlib.colormaps["plasma"]
        norm = matplotlib.colors.Normalize(vmin=valid.min() if valid.size else 0.0, vmax=np.max(gt_depth_np))
        panels = [
            (cmap(norm(gt_depth_np))[..., :3], "GT Depth"),
            (cmap(norm(depth_np))[..., :3], "Predicted Depth"),
            (depth_err_to_colorbar(depth_np, gt_depth_np, with_bar=False, cmap="jet")[..., :3], "Depth Residual"),
            (matplotlib.colormaps["gray"](uncertainty_np)[..., :3], "Uncertainty"),
            (gt_color_np.clip(0, 1), "GT RGB"),
            (color_np.clip(0, 1), "Predicted RGB"),
            (color_residual.clip(0, 1), "RGB Residual"),
            ((surface_normal / 255.0).clip(0, 1), "Surface Normal"),
        ]
        for ax, (im, title) in zip(axs.reshape(-1), panels):
            ax.imshow(im, cmap="plasma")
            ax.set_title(title, fontsize=8)
            ax.set_xticks([])
            ax.set_yticks([])
        fig.subplots_adjust(wspace=0, hspace=0)
        path = f"{self.vis_dir}/{idx:05d}.jpg"
        fig.savefig(path, bbox_inches="tight", pad_inches=0.2)
        print(f"INFO: Saved rendering visualization of color/depth image at {path}")
