"""Renderer.render_img / Visualizer.vis on the CPU: the oracle restatement (tests/render_img_restatement.py) against the
reference's own render_img (tests/golden/render_img.npz, tests/golden/gen_golden_render_img.py), the host-side depth
error colouring against the reference's, and the visualiser's plumbing with a stub renderer."""
import os

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def G():
    return {k: np.asarray(v) for k, v in np.load(os.path.join(HERE, "golden", "render_img.npz")).items()}


def _params(G):
    from oracle import neus_oracle as NO
    P = NO.make_params(int(G["seed"]), grid_init=0.3, bound=tuple(tuple(float(x) for x in r) for r in G["bound"]))
    P["rt_bound"] = torch.from_numpy(G["rt_bound"]).float()
    return P


@pytest.mark.parametrize("tag", ["a", "b"])
def test_restatement_matches_the_reference_render_img(G, tag):
    import render_img_restatement as RR
    P = _params(G)
    cam = [float(G[k]) for k in ("fx", "fy", "cx", "cy")]
    out = RR.render_img(P, int(G["H"]), int(G["W"]), *cam, G["c2w"], torch.from_numpy(G["gt_depth"]),
                        torch.from_numpy(G[f"perturb_{tag}"]), int(G[f"ray_batch_{tag}"]), int(G[f"points_batch_{tag}"]))
    g = {k: torch.from_numpy(G[f"{k}_{tag}"]) for k in out}
    assert out["gradient_error"].shape == g["gradient_error"].shape
    torch.testing.assert_close(out["z_vals"], g["z_vals"], rtol=1e-6, atol=1e-6)
    assert torch.equal(out["sdf"] == 100.0, g["sdf"] == 100.0), "in-bound masks (and the forced pieces) must agree"
    torch.testing.assert_close(out["sdf"], g["sdf"], rtol=1e-4, atol=2e-5)
    torch.testing.assert_close(out["weight_sum"], g["weight_sum"], rtol=0, atol=5e-4)
    torch.testing.assert_close(out["depth"], g["depth"], rtol=0, atol=2e-3)
    torch.testing.assert_close(out["depth_variance"], g["depth_variance"], rtol=1e-2, atol=2e-3)
    torch.testing.assert_close(out["color"].float(), g["color"].float(), rtol=0, atol=4e-3)
    torch.testing.assert_close(out["normal"], g["normal"], rtol=2e-3, atol=2e-3)
    torch.testing.assert_close(out["gradient_error"], g["gradient_error"], rtol=2e-3, atol=1e-5)
    torch.testing.assert_close(out["sdf_variance"], g["sdf_variance"])


def test_fixture_covers_the_cases_the_issue_names(G):
    """ragged last batch, pieces, zero depths, a batch without depth, a pixel at exactly 1e-3, empty pieces between
    non-empty ones (their first 100 points forced)"""
    n = int(G["H"]) * int(G["W"])
    assert n % int(G["ray_batch_a"]) and int(G["points_batch_a"]) < int(G["ray_batch_a"])
    gt = G["gt_depth"].reshape(-1)
    assert (gt == 0).any() and (gt == np.float32(1e-3)).sum() == 1
    assert any((gt[b:b + 300] == 0).all() for b in range(0, n, 300))
    inb = [(G["sdf_a"][r0:r0 + 128] != 100).sum() for r0 in (0, 300, 600, 900)]
    assert inb[0] > 100 and inb[1] == 100 and inb[2] == 100 and inb[3] > 100


@pytest.mark.parametrize("with_bar", [False, True])
def test_depth_err_to_colorbar_matches_the_reference(G, with_bar):
    from go_slam_amd.neus.image_vis import depth_err_to_colorbar
    H, W = int(G["H"]), int(G["W"])
    img = depth_err_to_colorbar(G["depth_a"].reshape(H, W), G["gt_depth"], with_bar=with_bar, cmap="jet")
    ref = G["depth_err_colorbar_bar" if with_bar else "depth_err_colorbar"]
    assert img.shape == ref.shape
    np.testing.assert_allclose(img, ref, rtol=0, atol=1e-12)


def test_visualizer_writes_the_figure_and_takes_both_pose_forms(G, tmp_path, monkeypatch, capsys):
    from go_slam_amd.neus import image_vis as V
    from go_slam_amd.neus.pose import quaternion_to_rt, rt_to_quaternion
    H, W = int(G["H"]), int(G["W"])
    seen = []

    class StubRenderer:
        def render_img(self, net, c2w, device, gt_depth=None):
            seen.append(torch.as_tensor(c2w).float().clone())
            return {k: torch.from_numpy(G[f"{k}_a"]) for k in ("color", "depth", "depth_variance", "normal",
                                                               "weight_sum", "sdf_variance", "sdf", "z_vals",
                                                               "gradient_error")}

    def metrics(render_out, gt_depth, gt_color, c2w):        # the HIP reduction is covered by the GPU tests
        imgs = {"normal_cam": torch.from_numpy(G["normal_cam"]), "depth_res": torch.from_numpy(G["depth_res"]),
                "color_res": torch.from_numpy(G["color_res"]).reshape(-1, 3)}
        return imgs, torch.tensor([float(G[f"metric_{k}"]) for k in ("mse", "psnr", "mae", "rmse", "s001", "s002")]
                                  + [1.0, 1.0], dtype=torch.float64)
    monkeypatch.setattr(V, "image_metrics", metrics)
    vis = V.Visualizer(str(tmp_path / "vis"), StubRenderer(), device="cpu")
    c2w = torch.from_numpy(G["c2w"])
    gd, gc = torch.from_numpy(G["gt_depth"]), torch.from_numpy(G["gt_color"])
    m = vis.vis(7, gd, gc, c2w, None)
    assert os.path.getsize(tmp_path / "vis" / "00007.jpg") > 0
    assert m["psnr"] == pytest.approx(float(G["metric_psnr"]))
    assert "MAE: %.4f" % float(G["metric_mae"]) in capsys.readouterr().out
    q = rt_to_quaternion(c2w)
    vis.vis(8, gd, gc, q, None)
    assert os.path.getsize(tmp_path / "vis" / "00008.jpg") > 0
    torch.testing.assert_close(seen[1], quaternion_to_rt(q))
    torch.testing.assert_close(seen[1], c2w, rtol=0, atol=1e-6)
    assert H * W == G["depth_a"].shape[0]
