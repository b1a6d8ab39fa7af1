"""The image-quality contract without a GPU: tests/image_quality_restatement.py against closed forms (so that the GPU
tests' reference is itself checked), the sharpness of its bound, the argument checks of go_slam_amd.neus.render_eval and
of the library (a refused size returns before anything is launched), and the round trip of metrics_render.txt."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import image_quality_restatement as IQ

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = IQ.U


def rgb(H, W, seed):
    return np.random.default_rng(seed).random((H, W, 3), dtype=np.float32)


# ---------------------------------------------------------------------------------------- the window ---------------
def test_weights_sum_to_one_and_are_symmetric():
    g = IQ.gaussian_window()
    assert g.dtype == np.float64 and g.shape == (11,)
    assert (g == g[::-1]).all()
    assert g.argmax() == 5 and (np.diff(g[:6]) > 0).all()
    # each g_k is within 14 u of e_k / sum (the restatement's WEIGHT_REL reasoning); adding 11 of them adds 11 u
    assert abs(math.fsum(g.tolist()) - 1.0) <= (14 + 11) * U
    w2 = g[:, None] * g[None, :]
    assert (w2 == w2.T).all()
    assert abs(math.fsum(w2.reshape(-1).tolist()) - 1.0) <= IQ.WEIGHT_REL + 121 * U
    # sigma 1.5: the ratio of neighbouring taps is exp((2 k - 11) / 4.5)
    assert g[4] / g[5] == pytest.approx(math.exp(-1 / 4.5), rel=1e-15)


def test_product_window_matches_render_eval():
    from go_slam_amd.neus import render_eval
    assert (render_eval.gaussian_window() == IQ.gaussian_window()).all()
    assert render_eval.QUALITY_KEYS == IQ.KEYS and render_eval.WINDOW == IQ.TAPS


# ---------------------------------------------------------------------------------------- closed forms -------------
@pytest.mark.parametrize("shape", [(11, 11), (13, 20)])
def test_identical_images(shape):
    x = rgb(*shape, seed=1)
    out, bound = IQ.image_quality(x, x.copy(), x[..., 0], x[..., 0].copy())
    assert out[0] == 0.0 and out[1] == math.inf and bound[1] == 0.0
    assert out[2] == 1.0
    assert out[3] == 0.0 and out[4] == (x[..., 0] > 0).sum()
    assert out[5] == 3 * (shape[0] - 10) * (shape[1] - 10) and out[6] == 0.0 and out[7] == 0.0


def test_two_constant_images():
    a, b = 0.25, 0.75                                    # exact in fp32
    x = np.full((12, 14, 3), a, dtype=np.float32)
    y = np.full((12, 14, 3), b, dtype=np.float32)
    out, bound = IQ.image_quality(x, y)
    want = (2 * a * b + IQ.C1) / (a * a + b * b + IQ.C1)  # the variances and the covariance vanish: C2 / C2
    print(f"ssim {out[2]!r} closed form {want!r} bound {bound[2]:.3e}")
    assert abs(out[2] - want) <= bound[2] + 4 * U * want
    assert 0 < bound[2] < 1e-9
    assert out[0] == 0.25 and abs(out[1] - (-10 * math.log10(0.25))) <= bound[1]
    assert math.isnan(out[3]) and out[4] == 0.0


def test_shifted_linear_ramp():
    """x = 1/4 + c / 64 along the columns, y = x + 1/8 (all exact in fp32): a symmetric window's mean is the value at
    its centre, and both variances and the covariance are (1/64)^2 sum g_k (k - 5)^2."""
    H, W = 12, 30
    col = np.arange(W, dtype=np.float64)
    x = np.broadcast_to((0.25 + col / 64)[None, :, None], (H, W, 3)).astype(np.float32)
    y = (x + np.float32(0.125)).astype(np.float32)
    assert (x.astype(np.float64) == 0.25 + col[None, :, None] / 64).all()
    m = IQ.window_moments(x, y)
    s, d_s, parts = IQ.ssim_map(m)
    g = IQ.gaussian_window()
    mu_x = np.broadcast_to((0.25 + (np.arange(W - 10) + 5) / 64)[None, :, None], (H - 10, W - 10, 3))
    mu_y = mu_x + 0.125
    var = math.fsum((g * (np.arange(11) - 5.0) ** 2).tolist()) / 4096
    assert (np.abs(m["x"] - mu_x) <= m["b_x"]).all() and (np.abs(m["y"] - mu_y) <= m["b_y"]).all()
    slack = 40 * U * var                                 # the closed form's own evaluation
    assert (np.abs(parts["vx"] - var) <= parts["d_vx"] + slack).all()
    assert (np.abs(parts["vy"] - var) <= parts["d_vy"] + slack).all()
    assert (np.abs(parts["cov"] - var) <= parts["d_cov"] + slack).all()
    assert (np.abs(parts["vx"] - parts["vy"]) <= parts["d_vx"] + parts["d_vy"]).all()
    want = (2 * mu_x * mu_y + IQ.C1) / (mu_x ** 2 + mu_y ** 2 + IQ.C1)     # 2 cov + C2 == var_x + var_y + C2
    assert (np.abs(s - want) <= d_s + 8 * U).all()
    assert d_s.max() < 1e-10
    out, bound = IQ.image_quality(x, y)
    assert abs(out[2] - want.mean()) <= bound[2] + 8 * U
    assert out[0] == 0.125 ** 2


def test_hand_computed_colour_error():
    x = np.zeros((11, 11, 3), dtype=np.float32)
    y = np.zeros((11, 11, 3), dtype=np.float32)
    x[0, 0, 0] = 0.5
    x[10, 10, 2] = -1.5                                  # nothing is clipped
    out, bound = IQ.image_quality(x, y)
    assert out[0] == (0.25 + 2.25) / 363
    assert abs(out[1] - (-10 * math.log10(2.5 / 363))) <= bound[1]
    assert out[5] == 3


def test_depth_error_by_hand():
    x = rgb(11, 11, seed=2)
    gt = np.zeros((11, 11), dtype=np.float32)
    pd = np.ones((11, 11), dtype=np.float32)
    gt[3, 4], gt[7, 1], gt[0, 0] = 2.0, 0.5, -1.0        # a negative depth is no measurement
    out, bound = IQ.image_quality(x, x, pd, gt)
    assert out[3] == 0.75 and out[4] == 2.0
    out, _ = IQ.image_quality(x, x, pd, np.zeros_like(gt))
    assert math.isnan(out[3]) and out[4] == 0.0


def test_nan_reaches_colour_sums_only():
    x, y = rgb(12, 12, seed=3), rgb(12, 12, seed=4)
    d = np.round(rgb(12, 12, seed=5)[..., 0] * 64 + 1) / np.float32(64)      # multiples of 1/64: d + 1/2 is exact
    x[5, 6, 1] = np.nan
    out, bound = IQ.image_quality(x, y, d, d + np.float32(0.5))
    assert math.isnan(out[0]) and math.isnan(out[1]) and math.isnan(out[2])
    assert abs(out[3] - 0.5) <= bound[3] and out[4] == 144


# ---------------------------------------------------------------------------------------- sharpness ----------------
def test_bound_catches_fp32_accumulation():
    """Window variances of 3e-7 under E[x^2] of 0.81: moments accumulated in fp32 leave the variance with no correct
    digit, and the index moves by far more than the fp64 bound allows.  A kernel that accumulated in fp32 would fail
    the GPU tests' tolerance (twice the bound).  The noise amplitude is 1e-3, at 11 x 12: it separates the two by a factor
    of about 1e6 (printed), so it was not lowered."""
    assert IQ.CANCEL_AMPLITUDE == 1e-3
    x, y = IQ.cancelling_pair()
    assert x.shape == (11, 12, 3)
    out64, bound = IQ.image_quality(x, y)
    out32, _ = IQ.image_quality(x, y, accumulate=np.float32)
    gap = abs(out32[2] - out64[2])
    print(f"ssim fp64 {out64[2]!r} fp32-accumulated {out32[2]!r} gap {gap:.3e} 2 x bound {2 * bound[2]:.3e}")
    assert gap > 2 * bound[2]
    assert gap > 1e3 * 2 * bound[2]                      # not a marginal separation
    assert bound[2] < 1e-9


# ---------------------------------------------------------------------------------------- arguments ----------------
def test_restatement_argument_checks():
    with pytest.raises(ValueError, match="smaller"):
        IQ.image_quality(rgb(10, 11, 0), rgb(10, 11, 0))
    with pytest.raises(ValueError, match="smaller"):
        IQ.image_quality(rgb(11, 10, 0), rgb(11, 10, 0))
    with pytest.raises(ValueError):
        IQ.image_quality(rgb(11, 11, 0), rgb(11, 12, 0))
    with pytest.raises(ValueError, match="both or neither"):
        IQ.image_quality(rgb(11, 11, 0), rgb(11, 11, 0), np.ones((11, 11), np.float32), None)


def test_python_argument_checks(built_lib):
    from go_slam_amd.neus.render_eval import image_quality
    a = torch.rand(11, 11, 3)
    with pytest.raises(ValueError, match="smaller"):
        image_quality(torch.rand(10, 11, 3), torch.rand(10, 11, 3))
    with pytest.raises(ValueError, match="smaller"):
        image_quality(torch.rand(1, 3, 11, 10), torch.rand(3, 11, 10))
    with pytest.raises(ValueError, match="differ"):
        image_quality(a, torch.rand(11, 12, 3))
    with pytest.raises(ValueError, match="both or neither"):
        image_quality(a, a, pred_depth=torch.rand(11, 11))
    with pytest.raises(ValueError, match="both or neither"):
        image_quality(a, a, gt_depth=torch.rand(11, 11))
    with pytest.raises(ValueError, match="depth"):
        image_quality(a, a, torch.rand(11, 12), torch.rand(11, 12))
    with pytest.raises(ValueError, match=r"\[H,W,3\]"):
        image_quality(torch.rand(11, 11), torch.rand(11, 11))
    with pytest.raises(RuntimeError, match="GPU tensor"):          # no CPU route
        image_quality(a, a)


def test_library_refuses_small_images_before_any_launch(built_lib):
    """H < 11 or W < 11 is the library's argument error; the check precedes every launch, so it runs without a GPU."""
    from go_slam_amd import _lib
    L = _lib.lib()
    fake = ctypes.c_void_p(256)                          # never dereferenced
    none = ctypes.c_void_p(0)
    for H, W in [(10, 11), (11, 10), (0, 640), (-3, 640)]:
        assert L.gs_image_quality_workspace_bytes(H, W) == 0
        assert L.gs_image_quality(fake, fake, none, none, H, W, fake, fake, 1 << 20, none) == -1      # GS_ERR_INVALID_ARG
        assert b"11 x 11" in L.gs_last_error()
    assert L.gs_image_quality(fake, fake, fake, none, 11, 11, fake, fake, 1 << 20, none) == -1        # half a depth pair
    assert L.gs_image_quality(fake, fake, none, none, 11, 11, fake, fake, 8, none) == -2              # GS_ERR_WORKSPACE


def test_tile_constants_and_workspace(built_lib):
    from go_slam_amd import _lib
    from go_slam_amd.neus import render_eval
    th, tw = render_eval.tile_shape()
    hdr = open(os.path.join(ROOT, "include", "goslam_neus.h")).read()
    assert th == int(re.search(r"#define GS_IQ_TILE_H (\d+)", hdr).group(1))
    assert tw == int(re.search(r"#define GS_IQ_TILE_W (\d+)", hdr).group(1))
    assert (th, tw) == IQ.TILE
    L = _lib.lib()
    assert L.gs_image_quality_workspace_bytes(11, 11) == 4 * 8
    for H, W in [(th + 10, tw + 10), (th + 11, tw + 11), (480, 640), (680, 1200)]:
        ty, tx = IQ.tiles(H, W, (th, tw))
        assert L.gs_image_quality_workspace_bytes(H, W) == tx * ty * 4 * 8


# ---------------------------------------------------------------------------------------- the report ---------------
def test_metrics_render_round_trip(tmp_path):
    from go_slam_amd.neus import render_eval as RE
    frames = [0, 5, 10, 15]
    per_frame = np.zeros((4, 8))
    per_frame[:, 1] = [0.1 + 0.2, 31.41592653589793, math.inf, 1e-300]
    per_frame[:, 2] = [1 / 3, 1.0, -0.25, 0.9999999999999999]
    per_frame[:, 3] = [0.012345678901234567, math.nan, 2.0 ** -40, math.nan]
    per_frame[:, 4] = [100, 0, 7, 0]
    result = RE.summarize(frames, per_frame)
    assert result["n_frames"] == 4 and result["psnr"] == math.inf
    assert result["ssim"] == (((1 / 3 + 1.0) + -0.25) + 0.9999999999999999) / 4
    assert result["depth_l1_cm"] == 100.0 * ((0.012345678901234567 + 2.0 ** -40) / 2)     # frames 5 and 15 left out
    path = tmp_path / "metrics_render.txt"
    path.write_text(RE.metrics_text(result, frames, per_frame))
    lines = path.read_text().splitlines()
    assert "PSNR" in lines[0] and "SSIM" in lines[0] and "valid windows" in lines[0] and "depth L1" in lines[1]
    assert [l.split("\t")[0] for l in lines[2:6]] == ["psnr", "ssim", "depth_l1_cm", "n_frames"]
    got, rows = RE.parse_metrics(path.read_text())
    assert got == result
    assert [r[0] for r in rows] == frames
    for r, want in zip(rows, per_frame):
        for a, b in zip(r[1:], want[1:4]):
            assert np.float64(a).tobytes() == np.float64(b).tobytes() or (math.isnan(a) and math.isnan(b))
    # no frame with depth: the mean is nan and the header says why in monocular mode
    per_frame[:, 4] = 0
    mono = RE.summarize(frames, per_frame)
    assert math.isnan(mono["depth_l1_cm"])
    text = RE.metrics_text(mono, frames, per_frame, metric_depth=False)
    assert "no metric scale" in text.splitlines()[1]
    assert math.isnan(RE.parse_metrics(text)[0]["depth_l1_cm"])
    with pytest.raises(ValueError):
        RE.parse_metrics("APE w.r.t. translation part (m)\n")
