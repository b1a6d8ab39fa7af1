#!/usr/bin/env python
"""Generate tests/golden/render_img.npz by RUNNING THE REFERENCE'S OWN Renderer.render_img and Visualizer.vis.

    python tests/golden/gen_golden_render_img.py        # needs the reference tree (as gen_golden.py does)

Reuses gen_golden.py's stand-ins by import (tinycudann over oracle/neus_oracle.py), so the reference's InstantNeuS runs
on the CPU with the oracle's hash grid and MLP.  cv2 is stubbed (the visualiser only imports it), and
`plt.cm.get_cmap` -- removed in matplotlib 3.9 -- is pointed at `matplotlib.colormaps`.  The perturbation rows are
recorded by wrapping `torch.rand`.

A 24 x 40 frame with
  * case "a": ray_batch_size 300 (960 = 3 x 300 + 60: a ragged last batch) and points_batch_size 128 (pieces of
    128, 128, 44 rays per batch), rendered through Visualizer.vis;
  * case "b": ray_batch_size 256, points_batch_size 10000 (one piece per batch), Renderer.render_img alone;
  * zero-depth pixels, a batch without any valid depth (pixels 600-899), a pixel at exactly 1e-3 (pixel 5);
  * a realtime bound that starts 1.3 in front of the camera: the batch of tiny depths (pixels 300-599) and the batch
    without depth have no point in it -- empty pieces between non-empty ones (the first 100 points forced valid).
Recorded: the rays, every output of render_img per case, the perturbation rows, the metrics (the reference's own expressions
from Visualizer.vis, checked against its printed line), the camera-frame normals (torch.inverse(c2w) as vis does)
and the `depth_err_to_colorbar` image."""
import contextlib
import importlib
import importlib.util
import io
import os
import re
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
SEED_NET = 227
H, W = 24, 40
CAM = dict(fx=30.0, fy=31.0, cx=19.5, cy=11.5)
BOUND = ((-2.5, 2.5), (-2.5, 2.5), (-2.5, 2.5))
RT_BOUND = ((-2.2, 2.3), (-2.4, 2.1), (-0.2, 2.2))
CASES = {"a": (300, 128), "b": (256, 10000)}


def load_gen():
    spec = importlib.util.spec_from_file_location("gen_golden", os.path.join(HERE, "gen_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def net_cfg():
    return {"sdf_network": {"d_in": 3, "d_out": 32},
            "color_network": {"d_in": 3, "d_feat": 31, "d_hidden": 64, "n_layers": 2},
            "variance_network": {"init_val": 0.2, "scale_factor": 10.0}, "sdf_smooth_std": 0.005,
            "sdf_sparse_factor": 5, "sdf_truncation": 0.16, "sdf_random_weight": 0.04}


def scene():
    """c2w, gt_depth [H,W], gt_color [H,W,3] (the tests read them back from the fixture)"""
    g = torch.Generator().manual_seed(229)
    a, b = 0.07, -0.05                          # a small rotation about y and x, camera 1.5 behind the origin
    Ry = torch.tensor([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], dtype=torch.float32)
    Rx = torch.tensor([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]], dtype=torch.float32)
    c2w = torch.eye(4)
    c2w[:3, :3] = Ry @ Rx
    c2w[:3, 3] = torch.tensor([0.1, -0.05, -1.5])
    depth = (torch.rand(H * W, generator=g) * 2.0 + 1.0)
    depth[300:600] = torch.rand(300, generator=g) * 0.25 + 0.05        # tiny depths: the whole batch out of bound
    depth[600:900] = 0.0                                                # a batch without valid depth
    depth[::11] = 0.0
    depth[5] = 1e-3
    color = torch.rand(H * W, 3, generator=g)
    return c2w, depth.reshape(H, W), color.reshape(H, W, 3)


def main():
    gen = load_gen()
    gen.install_stubs()
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    plt.cm.get_cmap = lambda name=None, lut=None: matplotlib.colormaps[name]
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    from oracle import neus_oracle as NO
    neus = importlib.import_module("refsrc.InstantNeuS")
    render = importlib.import_module("refsrc.render")
    vis_mod = importlib.import_module("refsrc.image_visualization")

    P = NO.make_params(SEED_NET, grid_init=0.3, bound=BOUND)
    torch.manual_seed(5)
    net = neus.InstantNeuS(net_cfg(), P["bound"].tolist(), device="cpu")
    with torch.no_grad():
        net.sdf_network.encoding.encoding.params.copy_(P["grid"])
        net.sdf_network.sdf_layer.weight.copy_(P["sdf_w"])
        net.sdf_network.sdf_layer.bias.copy_(P["sdf_b"])
        net.color_network._B.copy_(P["color_B"])
        net.color_network.network.params.copy_(P["mlp"])
        net.variance_network.variance.fill_(P["variance"])
    net.update_bound(torch.tensor(RT_BOUND))
    c2w, depth, color = scene()
    cfg = {"rendering": {"lindisp": False, "perturb": 1.0, "N_samples": 24, "N_surface": 48}}
    slam = types.SimpleNamespace(H=H, W=W, **CAM)

    rows = []
    real_rand = torch.rand

    def rand(*a, **k):
        t = real_rand(*a, **k)
        rows.append(t.clone())
        return t

    out = dict(seed=SEED_NET, c2w=c2w, gt_depth=depth, gt_color=color, bound=torch.tensor(BOUND),
               rt_bound=torch.tensor(RT_BOUND), H=H, W=W, **{k: np.float32(v) for k, v in CAM.items()})
    # the reference's rays themselves (a BLAS may round dirs @ R^T differently from one CPU to another)
    ro, rd = render.build_all_rays(H, W, CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"], c2w, "cpu", nerf_coordinate=False,
                                   dir_normalize=False)
    out.update(rays_o=ro.reshape(-1, 3), rays_d=rd.reshape(-1, 3))
    for tag, (B, Pb) in CASES.items():
        R = render.Renderer(cfg, None, slam, points_batch_size=Pb, ray_batch_size=B)
        out[f"ray_batch_{tag}"], out[f"points_batch_{tag}"] = B, Pb
        grabbed = {}
        orig = R.render_img

        def render_img(*a, **k):
            r = orig(*a, **k)
            grabbed.update(r)
            return r
        R.render_img = render_img
        rows.clear()
        torch.manual_seed(4000 + len(tag))
        torch.rand = rand
        try:
            if tag == "a":
                with tempfile.TemporaryDirectory() as d:
                    V = vis_mod.Visualizer(d, R, device="cpu")
                    buf = io.StringIO()
                    with contextlib.redirect_stdout(buf):
                        V.vis(3, depth, color, c2w, net)
                    printed = buf.getvalue()
                    assert os.path.exists(os.path.join(d, "00003.jpg"))
            else:
                R.render_img(net, c2w, "cpu", gt_depth=depth)
        finally:
            torch.rand = real_rand
        out[f"perturb_{tag}"] = torch.stack(rows)
        for k, v in grabbed.items():
            out[f"{k}_{tag}"] = v
        if tag == "a":
            # the reference's own expressions (image_visualization.py:57-86) on the outputs vis used
            gd, gc = depth.numpy(), color.numpy()
            dn = grabbed["depth"].reshape(H, W).numpy()
            cn = grabbed["color"].reshape(H, W, 3).numpy()
            mse = (np.abs(gc - cn) ** 2)[gd > 1e-3].mean()
            mae = (np.abs(gd - dn))[gd > 1e-3].mean()
            rmse = np.sqrt((np.abs(gd - dn) ** 2)[gd > 1e-3].mean())
            sdf = grabbed["sdf"]
            m = dict(mse=mse, psnr=-10.0 * np.log10(mse), mae=mae, rmse=rmse,
                     s001=float((torch.abs(sdf) < 0.01).float().mean()), s002=float((torch.abs(sdf) < 0.02).float().mean()))
            shown = [float(x) for x in re.findall(r"(?:MAE|PSNR|S0\.01|S0\.02): ([-0-9.na]+)", printed)]
            assert np.allclose(shown, [m["mae"], m["psnr"], m["s001"], m["s002"]], atol=6e-5), (printed, m)
            for k, v in m.items():
                out[f"metric_{k}"] = np.float64(v)
            w2c = torch.inverse(c2w)
            out["normal_cam"] = torch.matmul(w2c[None, :3, :3], grabbed["normal"][:, :, None])[..., 0]
            dres = np.abs(gd - dn)
            dres[gd < 1e-3] = 0.0
            cres = np.abs(gc - cn)
            cres[gd < 1e-3] = 0.0
            out["depth_res"], out["color_res"] = dres, cres
            out["depth_err_colorbar"] = vis_mod.depth_err_to_colorbar(dn, gd, with_bar=False, cmap="jet")
            out["depth_err_colorbar_bar"] = vis_mod.depth_err_to_colorbar(dn, gd, with_bar=True, cmap="jet")
            plt.close("all")
    gen.save("render_img.npz", **out)


if __name__ == "__main__":
    main()
