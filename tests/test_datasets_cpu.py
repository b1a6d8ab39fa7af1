"""The dataset readers' bookkeeping (go_slam_amd/datasets.py) against the reference's own classes (tests/golden/
datasets.npz, tests/golden/gen_golden_datasets.py), and the frame-preprocessing restatement (tests/
frame_prep_restatement.py) against torch's bilinear and grid_sample within one level.  No GPU needed."""
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import dataset_layouts as DL                     # noqa: E402
import frame_prep_restatement as R               # noqa: E402
from go_slam_amd import datasets as D            # noqa: E402

GOLD = np.load(os.path.join(HERE, "golden", "datasets.npz"))


@pytest.fixture(scope="module")
def parent(tmp_path_factory):
    return str(tmp_path_factory.mktemp("layouts"))


@pytest.mark.parametrize("case", list(DL.CASES))
def test_bookkeeping_matches_reference(case, parent):
    cfg, args = DL.build(case, parent)
    ds = D.get_dataset(cfg, args, device="cpu")
    rel = lambda ps: [os.path.relpath(p, parent) for p in ps]          # noqa: E731
    assert len(ds) == int(GOLD[f"{case}.n_img"])
    assert rel(ds.color_paths) == list(GOLD[f"{case}.color_paths"])
    if f"{case}.right_color_paths" in GOLD:
        assert rel(ds.right_color_paths) == list(GOLD[f"{case}.right_color_paths"])
    if f"{case}.depth_paths" in GOLD:
        assert rel(ds.depth_paths) == list(GOLD[f"{case}.depth_paths"])
    else:
        assert ds.depth_paths is None
    if f"{case}.poses" in GOLD:
        assert np.array_equal(np.stack(ds.poses), GOLD[f"{case}.poses"])
    else:
        assert ds.poses is None
    if f"{case}.image_timestamps" in GOLD:
        assert np.array_equal(np.asarray(ds.image_timestamps), GOLD[f"{case}.image_timestamps"])
    else:
        assert ds.image_timestamps is None
    for i in range(len(ds)):
        info = ds.frame_info(i)
        assert torch.equal(info["intrinsic"], torch.from_numpy(GOLD[f"{case}.intrinsic"][i]))
        if f"{case}.item_pose" in GOLD:
            assert torch.equal(info["pose"], torch.from_numpy(GOLD[f"{case}.item_pose"][i]))
        stereo = GOLD[f"{case}.color_levels"].shape[1] == 2
        assert len(info["color_paths"]) == (2 if stereo else 1)


def test_pixels_need_a_gpu(parent):
    cfg, args = DL.build("replica", parent)
    ds = D.get_dataset(cfg, args, device="cpu")
    with pytest.raises(RuntimeError, match="GPU"):
        ds[0]


def test_cofusion_is_refused():
    cfg = DL.CASES["replica"][2]
    with pytest.raises(NotImplementedError, match="EXR"):
        D.get_dataset({**cfg, "dataset": "cofusion"}, types.SimpleNamespace(input_folder="/nonexistent"), device="cpu")


def test_decoders(parent):
    cfg, args = DL.build("tum", parent)
    ds = D.get_dataset(cfg, args, device="cpu")
    d = D.read_depth(ds.depth_paths[0])
    assert d.dtype == np.uint16 and d.ndim == 2 and d.max() > 255
    c = D.read_color(ds.color_paths[0])
    assert c.dtype == np.uint8 and c.shape == (DL.H, DL.W, 3)
    cfg, args = DL.build("euroc", parent)
    g = D.read_color(D.get_dataset(cfg, args, device="cpu").color_paths[0])
    assert g.dtype == np.uint8 and g.shape == (480, 752)


def _bilinear(img, h, w):
    t = torch.from_numpy(img.astype(np.float32)).permute(2, 0, 1)[None]
    return F.interpolate(t, (h, w), mode="bilinear", align_corners=False, antialias=False)[0].permute(1, 2, 0).round()


@pytest.mark.parametrize("src,dst", [((680, 1200), (320, 640)), ((480, 640), (400, 528)), ((968, 1296), (256, 352)),
                                     ((30, 44), (71, 97)), ((240, 320), (480, 640)), ((1, 57), (4, 31)),
                                     ((45, 1), (12, 5)), ((1, 1), (3, 2)), ((64, 80), (32, 40))])
def test_resize_within_one_level_of_bilinear(src, dst):
    g = np.random.default_rng(src[0] * 7 + dst[1])
    img = g.integers(0, 256, src + (3,), dtype=np.uint8)
    out = torch.from_numpy(R.resize_u8(img, *dst).astype(np.float32))
    assert out.shape == (dst[0], dst[1], 3)
    assert float((out - _bilinear(img, *dst)).abs().max()) <= 1.0
    grey = R.resize_u8(img[:, :, 1], *dst)
    assert np.array_equal(grey, R.resize_u8(img, *dst)[:, :, 1])


def test_exact_2x_is_area():
    g = np.random.default_rng(3)
    img = g.integers(0, 256, (64, 80, 3), dtype=np.uint8)
    s = img.astype(np.int64)
    expect = (s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) >> 2
    assert np.array_equal(R.resize_u8(img, 32, 40), expect.astype(np.uint8))
    assert R.is_area_2x(64, 80, 32, 40) and not R.is_area_2x(64, 80, 32, 41)


def test_remap_within_one_level_of_grid_sample():
    g = np.random.default_rng(5)
    h, w = 37, 53
    img = g.integers(0, 256, (h, w, 3), dtype=np.uint8)
    yy, xx = np.meshgrid(np.arange(41, dtype=np.float32), np.arange(60, dtype=np.float32), indexing="ij")
    mx = (xx * 0.93 - 2.5 + g.normal(0, 0.7, xx.shape)).astype(np.float32)        # leaves the frame on both sides
    my = (yy * 0.97 - 1.7 + g.normal(0, 0.7, yy.shape)).astype(np.float32)
    # on OpenCV's 1/32-pixel grid: on a noise image the grid's rounding alone would move values by several levels
    mx, my = np.round(mx * 32) / 32, np.round(my * 32) / 32
    out = R.remap_u8(img, mx, my).astype(np.float32)
    grid = torch.from_numpy(np.stack([2 * mx / (w - 1) - 1, 2 * my / (h - 1) - 1], -1))[None]
    t = torch.from_numpy(img.astype(np.float32)).permute(2, 0, 1)[None]
    ref = F.grid_sample(t.double(), grid.double(), mode="bilinear", padding_mode="zeros", align_corners=True)
    ref = ref[0].permute(1, 2, 0).round().numpy()
    assert np.abs(out - ref).max() <= 1.0
    assert (out == 0).all(axis=2).sum() > 0                                       # some pixels are fully outside


def test_nearest_depth_resize_is_torch():
    g = np.random.default_rng(9)
    for (h, w), (H, W) in [((480, 640), (400, 528)), ((40, 56), (24, 32)), ((13, 17), (26, 34)), ((31, 7), (31, 9))]:
        d = g.integers(0, 65535, (h, w), dtype=np.uint16)
        ref = F.interpolate(torch.from_numpy(d.astype(np.float32) / 5000.0)[None, None], (H, W), mode="nearest")[0, 0]
        assert np.array_equal(R.depth_resize(d, 5000.0, H, W), ref.numpy())


def test_identity_map():
    K = np.array([[517.3, 0, 318.6], [0, 516.5, 255.3], [0, 0, 1]])
    mx, my = R.init_undistort_rectify_map(K, np.zeros(5), np.eye(3), K, (640, 480))
    yy, xx = np.meshgrid(np.arange(480, dtype=np.float32), np.arange(640, dtype=np.float32), indexing="ij")
    assert np.array_equal(mx, xx) and np.array_equal(my, yy)
    img = np.random.default_rng(1).integers(0, 256, (480, 640, 3), dtype=np.uint8)
    assert np.array_equal(R.remap_u8(img, mx, my), img)


def test_product_maps_are_the_restatement():
    for (K, Dc, Rm, P), (mx, my) in zip(D.EUROC_RECT, D.euroc_maps()):
        rx, ry = R.init_undistort_rectify_map(K, Dc, Rm, P[:3, :3], D.EUROC_SIZE)
        assert mx.dtype == np.float32 and mx.shape == (480, 752)
        assert np.array_equal(mx, rx) and np.array_equal(my, ry)
    K = np.array([[30.0, 0, 27.5], [0, 31.0, 19.5], [0, 0, 1]])
    dist = np.array([0.1, -0.05, 0.001, 0.002])
    assert all(np.array_equal(a, b) for a, b in zip(D.init_undistort_rectify_map(K, dist, np.eye(3), K, (56, 40)),
                                                    R.undistort_maps(K, dist, (56, 40))))


def test_dropin_datasets_keyword():
    from go_slam_amd import dropin
    saved = {k: sys.modules.get(k) for k in ("droid_backends", "tinycudann", "lietorch", "torch_scatter",
                                              "src.datasets")}
    try:
        sys.modules.pop("src.datasets", None)
        dropin.install()
        assert "src.datasets" not in sys.modules
        dropin.install(datasets=True)
        assert sys.modules["src.datasets"] is D
        assert sys.modules["src.datasets"].get_dataset is D.get_dataset
        assert set(D.dataset_dict) == {"replica", "scannet", "cofusion", "azure", "tumrgbd", "eth3d", "euroc"}
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
