"""gs_image_quality on the GPU against tests/image_quality_restatement.py, every output within TWICE the restatement's
own forward-error bound (both sides obey it against the exact value) and the counts exactly; then eval_rendering on a
small random map, and one whole SLAM run with `render_eval` switched on.

The sizes are the smallest at which the kernel takes another path: one window; one row and one column of windows; two
tiles each way with a ragged second tile (from the tile shape the library reports); three tiles each way, so that one
tile has neighbours on every side."""
import math
import os
import types

import numpy as np
import pytest
import torch

import image_quality_restatement as IQ

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def RE(built_lib):
    from go_slam_amd.neus import render_eval
    return render_eval


def images(H, W, seed, lo=0.0, hi=1.0):
    r = np.random.default_rng(seed)
    x = (lo + (hi - lo) * r.random((H, W, 3))).astype(np.float32)
    y = (lo + (hi - lo) * r.random((H, W, 3))).astype(np.float32)
    return x, y


def depths(H, W, seed, zero_fraction):
    r = np.random.default_rng(seed)
    gt = (0.5 + 3.5 * r.random((H, W))).astype(np.float32)
    gt[r.random((H, W)) < zero_fraction] = 0.0
    pred = (gt + 0.1 * r.standard_normal((H, W))).astype(np.float32)
    return pred, gt


def run_gpu(RE, x, y, pd=None, gd=None):
    t = [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (x, y, pd, gd)]
    out = RE.image_quality(*t)
    assert out.dtype == torch.float64 and out.shape == (8,) and out.is_cuda
    return out.cpu().numpy()


def compare(got, want, bound, label):
    for k in range(4):
        print(f"{label} {IQ.KEYS[k]}: gpu {got[k]!r} restatement {want[k]!r} diff {abs(got[k] - want[k]):.3e} "
              f"2 x bound {2 * bound[k]:.3e}")
    for k in range(4):
        if math.isnan(want[k]):
            assert math.isnan(got[k]), IQ.KEYS[k]
        elif math.isinf(want[k]):
            assert got[k] == want[k], IQ.KEYS[k]
        else:
            assert math.isfinite(bound[k]) and abs(got[k] - want[k]) <= 2 * bound[k], IQ.KEYS[k]
    assert got[4] == want[4] and got[5] == want[5] and got[6] == 0.0 and got[7] == 0.0


def ragged_size(RE):
    """window positions: tile edge + 1 rows, tile edge + tile / 2 + 3 columns -- two tiles each way, both ragged"""
    th, tw = RE.tile_shape()
    return th + 1 + 10, tw + tw // 2 + 3 + 10


def test_tile_shape_is_the_restatements(RE):
    assert RE.tile_shape() == IQ.TILE


@pytest.mark.parametrize("shape", [(11, 11), (11, 29), (29, 11), "ragged", "three_tiles"])
def test_random_images(RE, shape):
    th, tw = RE.tile_shape()
    H, W = {"ragged": ragged_size(RE), "three_tiles": (2 * th + 5 + 10, 2 * tw + 7 + 10)}.get(shape, shape)
    x, y = images(H, W, seed=H * 1000 + W)
    pd, gd = depths(H, W, seed=7, zero_fraction=0.3)
    want, bound = IQ.image_quality(x, y, pd, gd, tile=(th, tw))
    got = run_gpu(RE, x, y, pd, gd)
    compare(got, want, bound, f"{H}x{W}")
    assert got[5] == 3 * (H - 10) * (W - 10) and got[4] == (gd > 0).sum() and 0 < got[4] < H * W
    assert bound[2] < 1e-9 and bound[0] < 1e-12          # the tolerance is an fp64 one


def test_cancelling_input(RE):
    """0.9 plus noise of amplitude 1e-3: the input on which fp32 moments fail the bound
    (test_image_quality_cpu.test_bound_catches_fp32_accumulation)"""
    H, W = ragged_size(RE)
    for shape in [(11, 12), (H, W)]:
        x, y = IQ.cancelling_pair(*shape)
        want, bound = IQ.image_quality(x, y, tile=RE.tile_shape())
        compare(run_gpu(RE, x, y), want, bound, f"cancelling {shape}")
        assert bound[2] < 1e-9


def test_identical_images(RE):
    H, W = ragged_size(RE)
    x, _ = images(H, W, seed=11)
    pd, _ = depths(H, W, seed=12, zero_fraction=0.0)
    got = run_gpu(RE, x, x.copy(), pd, pd.copy())
    assert got[0] == 0.0 and got[1] == math.inf and got[2] == 1.0 and got[3] == 0.0
    assert got[4] == H * W and got[5] == 3 * (H - 10) * (W - 10)


def test_depth_cases(RE):
    H, W = ragged_size(RE)
    x, y = images(H, W, seed=13)
    pd, gd = depths(H, W, seed=14, zero_fraction=0.3)
    tile = RE.tile_shape()
    base = run_gpu(RE, x, y, pd, gd)
    none = run_gpu(RE, x, y)
    zeros = run_gpu(RE, x, y, pd, np.zeros_like(gd))
    compare(zeros, *IQ.image_quality(x, y, pd, np.zeros_like(gd), tile=tile), "all-zero depth")
    compare(none, *IQ.image_quality(x, y, tile=tile), "no depth")
    for got in (none, zeros):
        assert math.isnan(got[3]) and got[4] == 0.0
        assert got[:3].tobytes() == base[:3].tobytes()   # the colour outputs do not depend on the depth pair
    # a NaN or negative measurement is no measurement; a NaN prediction at a measured pixel is reported
    gd2 = gd.copy()
    gd2[0, 0], gd2[H - 1, W - 1] = np.nan, -1.0
    compare(run_gpu(RE, x, y, pd, gd2), *IQ.image_quality(x, y, pd, gd2, tile=tile), "nan / negative gt depth")
    pd2 = pd.copy()
    r, c = np.argwhere(gd > 0)[5]
    pd2[r, c] = np.nan
    assert math.isnan(run_gpu(RE, x, y, pd2, gd)[3])


def test_single_nan_pixel(RE):
    H, W = ragged_size(RE)
    x, y = images(H, W, seed=15)
    pd, gd = depths(H, W, seed=16, zero_fraction=0.3)
    clean = run_gpu(RE, x, y, pd, gd)
    for (r, c, ch) in [(H // 2, W // 2, 1), (H - 1, W - 1, 2)]:      # the second one only the last tile's apron holds
        xn = x.copy()
        xn[r, c, ch] = np.nan
        got = run_gpu(RE, xn, y, pd, gd)
        assert math.isnan(got[0]) and math.isnan(got[1]) and math.isnan(got[2])
        assert got[3:].tobytes() == clean[3:].tobytes()
        compare(got, *IQ.image_quality(xn, y, pd, gd, tile=RE.tile_shape()), "nan pixel")


def test_values_outside_the_unit_range(RE):
    H, W = ragged_size(RE)
    x, y = images(H, W, seed=17, lo=-2.0, hi=3.0)
    want, bound = IQ.image_quality(x, y, tile=RE.tile_shape())
    got = run_gpu(RE, x, y)
    compare(got, want, bound, "range [-2, 3]")
    assert got[1] < 0                                    # an error above the data range: nothing was clipped


def test_planar_input_and_repeatability(RE):
    H, W = ragged_size(RE)
    x, y = images(H, W, seed=18)
    pd, gd = depths(H, W, seed=19, zero_fraction=0.3)
    tx, ty, tp, tg = (torch.from_numpy(a).to(DEV) for a in (x, y, pd, gd))
    a = RE.image_quality(tx, ty, tp, tg).cpu().numpy()
    b = RE.image_quality(tx, ty, tp, tg).cpu().numpy()
    assert a.tobytes() == b.tobytes()
    planar = RE.image_quality(tx.permute(2, 0, 1).contiguous(), ty.permute(2, 0, 1).contiguous()[None], tp, tg)
    assert planar.cpu().numpy().tobytes() == a.tobytes()
    view = RE.image_quality(tx.permute(2, 0, 1).contiguous().permute(1, 2, 0), ty, tp.reshape(-1), tg.reshape(-1, 1))
    assert view.cpu().numpy().tobytes() == a.tobytes()


# ---------------------------------------------------------------------------------------- eval_rendering -----------
EH, EW = 24, 32


class ListStream:
    """five in-memory frames with the dataset items' layout"""

    def __init__(self, n=5):
        g = torch.Generator().manual_seed(21)
        self.color = torch.rand(n, 1, 3, EH, EW, generator=g)
        self.depth = torch.rand(n, EH, EW, generator=g) * 2.0 + 1.0
        self.depth[:, 3, 4] = 0.0
        self.c2w = torch.eye(4).repeat(n, 1, 1)
        self.c2w[:, 0, 3] = torch.linspace(-0.2, 0.2, n)
        self.input_folder, self.poses = "list", None

    def __len__(self):
        return self.color.shape[0]

    def __getitem__(self, i):
        return i, self.color[i].clone(), self.depth[i].clone(), torch.tensor([28.8, 28.8, 15.5, 11.5]), self.c2w[i].clone()


class RenderRecorder:
    def __init__(self, renderer):
        self.inner, self.calls = renderer.render_img, []

    def __call__(self, net, c2w, device, gt_depth=None):
        self.calls.append((c2w.clone(), None if gt_depth is None else gt_depth.clone()))
        return self.inner(net, c2w, device, gt_depth=gt_depth)


@pytest.fixture(scope="module")
def small_map(built_lib):
    import go_slam_amd.neus as neus
    torch.manual_seed(5)
    model = neus.InstantNeuS({}, [[-2.5, 2.5], [-2.5, 2.5], [-1.0, 4.0]], device=DEV).to(DEV)
    R = neus.Renderer(N_samples=24, N_surface=48, ray_batch_size=300, points_batch_size=500, H=EH, W=EW, fx=28.8, fy=28.8,
                      cx=15.5, cy=11.5)
    return model, R


@pytest.mark.parametrize("mode", ["rgbd", "mono"])
def test_eval_rendering(RE, small_map, tmp_path, mode):
    model, R = small_map
    stream = ListStream()
    slam = types.SimpleNamespace(renderer=types.SimpleNamespace(render_img=RenderRecorder(R)), mapping_net=model,
                                 mode=mode)
    path = tmp_path / "metrics_render.txt"
    torch.manual_seed(31)
    res = RE.eval_rendering(slam, stream, stream.c2w, every=2, out_path=str(path), save_images=(mode == "rgbd"))
    assert res["frames"] == [0, 2, 4] and res["n_frames"] == 3 and res["per_frame"].shape == (3, 8)
    calls = slam.renderer.render_img.calls
    assert len(calls) == 3
    # the same frames again under the same seed, by hand
    torch.manual_seed(31)
    want = []
    for (c2w, gt_depth), i in zip(calls, (0, 2, 4)):
        assert torch.equal(c2w, stream.c2w[i])
        if mode == "rgbd":
            assert torch.equal(gt_depth.cpu(), stream.depth[i])
        else:
            assert gt_depth is None
        out = R.render_img(model, stream.c2w[i], DEV, gt_depth=stream.depth[i].to(DEV) if mode == "rgbd" else None)
        pair = (out["depth"].reshape(EH, EW), stream.depth[i].to(DEV)) if mode == "rgbd" else (None, None)
        want.append(RE.image_quality(out["color"].reshape(EH, EW, 3), stream.color[i].to(DEV), *pair).cpu().numpy())
    want = np.stack(want)
    assert want.tobytes() == res["per_frame"].tobytes()
    summary, rows = RE.parse_metrics(path.read_text())
    assert [r[0] for r in rows] == [0, 2, 4]
    for r, w in zip(rows, want):
        assert np.array(r[1:], dtype=np.float64).tobytes() == w[1:4].tobytes()
    assert np.isfinite(want[:, 1:3]).all() and (want[:, 5] == 3 * (EH - 10) * (EW - 10)).all()

    def mean(vals):
        total = 0.0
        for v in vals:
            total += v
        return total / len(vals)
    assert summary["psnr"] == mean([r[1] for r in rows]) == res["psnr"]
    assert summary["ssim"] == mean([r[2] for r in rows]) == res["ssim"]
    assert summary["n_frames"] == 3
    if mode == "rgbd":
        assert (want[:, 4] == EH * EW - 1).all()
        assert summary["depth_l1_cm"] == 100.0 * mean([r[3] for r in rows]) == res["depth_l1_cm"]
        assert sorted(os.listdir(tmp_path / "render_eval")) == ["00000.jpg", "00002.jpg", "00004.jpg"]
        from PIL import Image
        with Image.open(tmp_path / "render_eval" / "00002.jpg") as im:
            assert im.size == (2 * EW, EH)
    else:
        assert np.isnan(want[:, 3]).all() and (want[:, 4] == 0).all() and math.isnan(summary["depth_l1_cm"])
        assert "no metric scale" in path.read_text().splitlines()[1]
        assert not os.path.exists(tmp_path / "render_eval")


# ---------------------------------------------------------------------------------------- a whole run --------------
N, H, W = 16, 64, 96        # the size of tests/test_slam_gpu.py's runs, built by the same recipe


def make_cfg(out_dir):
    return {
        "sync_method": "strict", "verbose": False, "dataset": "synthetic", "mode": "rgbd", "stride": 1,
        "only_tracking": False,
        "mapping": {"device": DEV, "BA": False, "BA_cam_lr": 0.001, "net_lr": 0.001, "grid_lr": 0.01,
                    "w_color_loss": 2.0, "w_sdf_smooth_loss": 1.0, "w_sdf_loss": 2.0, "w_eikonal_loss": 0.1,
                    "uncertainty_weight_loss": True, "mapping_window_size": 22, "pixels": 512, "iters": 2,
                    "post_processing_iters": 2, "decay": 0.8, "bound": [[-4.0, 4.0], [-3.0, 2.0], [-1.0, 5.0]],
                    "model": {"sdf_smooth_std": 0.005, "sdf_sparse_factor": 5, "sdf_truncation": 0.16,
                              "sdf_random_weight": 0.04, "sdf_network": {"d_in": 3, "d_out": 32},
                              "color_network": {"d_in": 3, "d_feat": 31, "d_hidden": 64, "n_layers": 2},
                              "variance_network": {"init_val": 0.2, "scale_factor": 10.0}}},
        "tracking": {"device": DEV, "pretrained": None, "buffer": 32, "beta": 0.75, "warmup": 8, "upsample": True,
                     "motion_filter": {"thresh": 0.0},
                     "multiview_filter": {"thresh": 0.05, "visible_num": 2, "kernel_size": 1, "bound_enlarge_scale": 1.10},
                     "frontend": {"enable_loop": True, "keyframe_thresh": 0.0, "thresh": 1e4, "window": 25, "radius": 1,
                                  "nms": 1, "max_factors": 75},
                     "backend": {"thresh": 1e4, "radius": 1, "nms": 5, "loop_window": 25, "loop_thresh": 1e4,
                                 "loop_radius": 1, "loop_nms": 12}},
        "cam": {"H": H, "W": W, "fx": 0.9 * W, "fy": 0.9 * W, "cx": W / 2 - 0.5, "cy": H / 2 - 0.5,
                "png_depth_scale": 1000.0, "calibration_txt": "", "H_edge": 0, "W_edge": 0, "H_out": H, "W_out": W},
        "rendering": {"N_samples": 24, "N_surface": 48, "lindisp": False, "perturb": 1.0},
        "data": {"input_folder": "synthetic", "output": out_dir, "video_length": ""},
        "meshing": {"level_set": 0, "resolution": 32, "eval_rec": False, "get_largest_components": False,
                    "remove_small_geometry_threshold": 0.2, "n_points_to_eval": 200000, "mesh_threshold_to_eval": 0.05,
                    "gt_mesh_path": "", "forecast_radius": 0},
        "render_eval": {"enable": True, "every": 4},
    }


def test_whole_run_writes_metrics_render(RE, tmp_path):
    import random
    from go_slam_amd import synth
    from go_slam_amd.slam import SLAM
    torch.manual_seed(43)
    torch.cuda.manual_seed_all(43)
    np.random.seed(43)
    random.seed(43)
    out_dir = str(tmp_path / "with_key")
    cfg = make_cfg(out_dir)
    args = types.SimpleNamespace(device=DEV, make_video=False, output=None)
    slam = SLAM(args, cfg, full_ba_every=4)
    with torch.no_grad():       # small output heads: a random network must not throw the poses to infinity
        slam.net.update.delta[2].weight.mul_(0.02)
        slam.net.update.delta[2].bias.zero_()
    slam.ba.frontend_window = 8
    stream = synth.PlaneSequence(N, H, W, 0.9 * W, 0.9 * W, W / 2 - 0.5, H / 2 - 0.5, poses=True, timestamps=False)
    slam.run(stream)
    recorder = RenderRecorder(slam.renderer)
    slam.renderer.render_img = recorder
    stats = slam.terminate(rank=-1, stream=stream)
    torch.cuda.synchronize()

    summary, rows = RE.parse_metrics(open(f"{out_dir}/metrics_render.txt").read())
    assert [r[0] for r in rows] == [0, 4, 8, 12] and summary["n_frames"] == 4 and len(recorder.calls) == 4
    poses = torch.from_numpy(np.load(f"{out_dir}/checkpoints/est_poses.npy"))
    for (c2w, gt_depth), i in zip(recorder.calls, (0, 4, 8, 12)):
        assert torch.equal(c2w, poses[i]) and gt_depth is not None       # the poses of the file, as the mesher's
    for _, psnr, ssim, depth_l1 in rows:
        print(f"psnr {psnr!r} ssim {ssim!r} depth_l1 {depth_l1!r}")
        assert math.isfinite(psnr) and -1.0 < ssim <= 1.0 and math.isfinite(depth_l1)
    assert math.isfinite(summary["psnr"]) and -1.0 < summary["ssim"] <= 1.0
    for k in ("psnr", "ssim", "depth_l1_cm", "n_frames"):
        assert stats[f"render_{k}"] == summary[k]
    assert "rmse" in stats and os.path.exists(f"{out_dir}/mesh/final_raw_mesh.ply")     # the rest of terminate ran

    # the same run's terminate without the key, disabled, and under only_tracking: no render, no file, no keys
    for name, edit in [("absent", lambda c: c.pop("render_eval")),
                       ("disabled", lambda c: c.update(render_eval={"enable": False, "every": 4})),
                       ("only_tracking", lambda c: c.update(render_eval={"enable": True, "every": 4}))]:
        edit(slam.cfg)
        slam.output = str(tmp_path / name)
        slam.only_tracking = name == "only_tracking"
        os.makedirs(slam.output, exist_ok=True)
        stats = slam.terminate(rank=-1, stream=stream)
        assert len(recorder.calls) == 4, name
        assert not os.path.exists(f"{slam.output}/metrics_render.txt"), name
        assert not any(k.startswith("render_") for k in stats) and "rmse" in stats, name
