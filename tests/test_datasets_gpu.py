"""The frame preprocessing kernels (csrc/frame_prep.hip) against tests/frame_prep_restatement.py bit for bit, and the
dataset readers' items against the reference's own classes (tests/golden/datasets.npz) bit for bit, on the MI355X."""
import os
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import dataset_layouts as DL                     # noqa: E402
import frame_prep_restatement as R               # noqa: E402
from go_slam_amd import _lib                     # noqa: E402
from go_slam_amd import datasets as D            # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = np.load(os.path.join(HERE, "golden", "datasets.npz"))


def prep_color(imgs, H_out, W_out, H_edge, W_edge, maps=None):
    """The kernel on uint8 RGB [h,w,3] / grey [h,w] host arrays (all views in one call) -> [n,3,H_out,W_out] host."""
    dev = torch.device(DEV)
    srcs = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in imgs]
    out = torch.full((len(imgs), 3, H_out, W_out), float("nan"), device=dev)
    keep, views = [], []
    for k, (a, s) in enumerate(zip(imgs, srcs)):
        v = _lib.ColorView(src=s.data_ptr(), dst=out[k].data_ptr(), h=a.shape[0], w=a.shape[1],
                           c=1 if a.ndim == 2 else 3)
        if maps is not None and maps[k] is not None:
            mx, my = (torch.from_numpy(m).to(dev) for m in maps[k])
            tmp = torch.empty(mx.numel() * v.c + 4, dtype=torch.uint8, device=dev)
            keep += [mx, my, tmp]
            v.map_x, v.map_y, v.tmp, v.mh, v.mw = mx.data_ptr(), my.data_ptr(), tmp.data_ptr(), *mx.shape
        views.append(v)
    arr = (_lib.ColorView * len(views))(*views)
    _lib.check(_lib.lib().gs_frame_prep_color(arr, len(views), H_out, W_out, H_edge, W_edge, _lib.stream_ptr(dev)),
               "gs_frame_prep_color")
    return out.cpu().numpy()


def prep_depth(deps, scale, H_out, W_out, H_edge, W_edge):
    dev = torch.device(DEV)
    srcs = [torch.from_numpy(d.astype(np.int32)).to(dev).to(torch.uint16) for d in deps]
    out = torch.full((len(deps), H_out, W_out), float("nan"), device=dev)
    views = [_lib.DepthView(src=s.data_ptr(), dst=out[k].data_ptr(), h=d.shape[0], w=d.shape[1])
             for k, (d, s) in enumerate(zip(deps, srcs))]
    arr = (_lib.DepthView * len(views))(*views)
    _lib.check(_lib.lib().gs_frame_prep_depth(arr, len(views), float(scale), H_out, W_out, H_edge, W_edge,
                                              _lib.stream_ptr(dev)), "gs_frame_prep_depth")
    return out.cpu().numpy()


def expect_color(img, H_out, W_out, H_edge, W_edge, maps=None):
    bgr = img if img.ndim == 2 else img[:, :, ::-1]          # the decoder's RGB is cv2.imread's BGR reversed
    return R.color_item(bgr, H_out, W_out, H_edge, W_edge, maps)


# (source h, w), (H_out, W_out, H_edge, W_edge): every shipped config, then odd sizes, upscales, 1-pixel frames, 2x
SHAPES = [((680, 1200), (320, 640, 0, 0)), ((480, 640), (384, 512, 8, 8)), ((968, 1296), (240, 320, 8, 16)),
          ((480, 640), (240, 320, 8, 16)), ((458, 739), (384, 512, 8, 8)), ((480, 752), (384, 512, 8, 8)),
          ((480, 752), (320, 480, 8, 8)), ((37, 53), (23, 31, 1, 2)), ((20, 30), (57, 91, 0, 3)),
          ((1, 57), (4, 31, 1, 0)), ((45, 1), (12, 5, 0, 2)), ((64, 80), (32, 40, 0, 0)), ((72, 88), (32, 40, 2, 2)),
          ((99, 131), (99, 131, 0, 0))]


@pytest.mark.parametrize("src,out", SHAPES)
def test_color_kernel_is_the_restatement(src, out, built_lib):
    g = np.random.default_rng(src[0] * 31 + out[1])
    imgs = [g.integers(0, 256, src + (3,), dtype=np.uint8), g.integers(0, 256, src, dtype=np.uint8)]
    got = prep_color(imgs, *out)
    for k, img in enumerate(imgs):
        assert np.array_equal(got[k], expect_color(img, *out)), k


@pytest.mark.parametrize("src,out", SHAPES)
def test_depth_kernel_is_the_restatement(src, out, built_lib):
    g = np.random.default_rng(src[1] * 17 + out[0])
    deps = [g.integers(0, 65536, src, dtype=np.uint16) for _ in range(2)]
    for scale in (5000.0, 6553.5, 1000.0):
        got = prep_depth(deps, scale, *out)
        for k, d in enumerate(deps):
            assert np.array_equal(got[k], R.depth_item(d, scale, *out)), (k, scale)


def test_mixed_batch_in_one_call(built_lib):
    """views of different sizes and channel counts, more than one launch's worth"""
    g = np.random.default_rng(7)
    sizes = [(40 + 3 * k, 56 + 5 * k) for k in range(_lib.FRAME_PREP_MAX_VIEWS + 5)]
    imgs = [g.integers(0, 256, s + ((3,) if k % 3 else ()), dtype=np.uint8) for k, s in enumerate(sizes)]
    got = prep_color(imgs, 24, 40, 2, 4)
    for k, img in enumerate(imgs):
        assert np.array_equal(got[k], expect_color(img, 24, 40, 2, 4)), k


@pytest.mark.parametrize("out", [(384, 512, 8, 8), (320, 480, 8, 8)])
def test_euroc_rectification_is_the_restatement(out, built_lib):
    g = np.random.default_rng(11)
    maps = D.euroc_maps()
    imgs = [g.integers(0, 256, (480, 752), dtype=np.uint8) for _ in range(2)]
    imgs.append(g.integers(0, 256, (480, 752, 3), dtype=np.uint8))
    got = prep_color(imgs, *out, maps=[maps[0], maps[1], maps[1]])
    for k, img in enumerate(imgs):
        assert np.array_equal(got[k], expect_color(img, *out, maps=maps[min(k, 1)])), k


def test_undistort_path_is_the_restatement(built_lib, tmp_path):
    cfg, args = DL.build("tum", str(tmp_path))
    cfg = {**cfg, "cam": {**cfg["cam"], "distortion": [0.12, -0.21, 0.001, -0.002, 0.05]}}
    ds = D.get_dataset(cfg, args, device=DEV, output="device")
    K = np.array([[ds.fx, 0, ds.cx], [0, ds.fy, ds.cy], [0, 0, 1]])
    for i in range(2):
        _, color, _, _, _ = ds[i]
        img = D.read_color(ds.color_paths[i])
        maps = R.undistort_maps(K, np.array(cfg["cam"]["distortion"]), (img.shape[1], img.shape[0]))
        assert np.array_equal(color[0].cpu().numpy(), expect_color(img, 24, 40, 2, 4, maps))


def _check_items(case, items):
    levels = GOLD[f"{case}.color_levels"]
    assert len(items) == levels.shape[0]
    for i, (index, color, depth, intr, pose) in enumerate(items):
        assert index == i
        expect = torch.from_numpy(levels[i]).float() / 255.0
        assert torch.equal(color.cpu(), expect), (case, i)
        if f"{case}.depth" in GOLD:
            assert torch.equal(depth.cpu(), torch.from_numpy(GOLD[f"{case}.depth"][i])), (case, i)
        else:
            assert depth is None
        assert torch.equal(intr, torch.from_numpy(GOLD[f"{case}.intrinsic"][i]))
        if f"{case}.item_pose" in GOLD:
            assert torch.equal(pose, torch.from_numpy(GOLD[f"{case}.item_pose"][i]))


@pytest.fixture(scope="module")
def parent(tmp_path_factory):
    return str(tmp_path_factory.mktemp("layouts"))


@pytest.mark.parametrize("case", list(DL.CASES))
def test_items_equal_the_reference(case, parent, built_lib):
    cfg, args = DL.build(case, parent)
    dev_ds = D.get_dataset(cfg, args, device=DEV, output="device")
    items = [dev_ds[i] for i in range(len(dev_ds))]
    assert all(it[1].is_cuda for it in items)
    _check_items(case, items)
    # the prefetching iterator, host output (the default), batches of 3 frames on 2 decoder threads
    host_ds = D.get_dataset(cfg, args, device=DEV, decode_threads=2, batch=3)
    items = list(host_ds)
    assert all(it[1].device.type == "cpu" and (it[2] is None or it[2].device.type == "cpu") for it in items)
    _check_items(case, items)
    # load_batch: one colour and one depth launch for all of them
    _check_items(case, host_ds.load_batch(list(range(len(host_ds)))))


def test_items_do_not_share_storage(parent, built_lib):
    cfg, args = DL.build("tum", parent)
    for output in ("host", "device"):
        ds = D.get_dataset(cfg, args, device=DEV, output=output, batch=2)
        items = list(ds)
        ptrs = [p for it in items for p in (it[1].data_ptr(), it[2].data_ptr())]
        assert len(set(ptrs)) == len(ptrs), output
    assert D.get_dataset(cfg, args, device=DEV)[0][1].device.type == "cpu"


def _video_cfg(H_out, W_out):
    return {"verbose": False, "mode": "rgbd", "cam": {"H_out": H_out, "W_out": W_out}, "tracking": {
        "buffer": 16, "warmup": 8, "upsample": True, "beta": 0.75,
        "frontend": {"max_factors": 75, "nms": 1, "keyframe_thresh": 0.05, "window": 10, "thresh": 1e4, "radius": 2,
                     "enable_loop": False},
        "backend": {"thresh": 1e4, "radius": 1, "nms": 2, "loop_window": 8, "loop_thresh": 1e4, "loop_radius": 1,
                    "loop_nms": 2},
        "multiview_filter": {"thresh": 0.2, "visible_num": 2, "kernel_size": 3, "bound_enlarge_scale": 1.1}}}


def test_motion_filter_stores_unnormalised_images(parent, built_lib):
    """The default host output feeds MotionFilter.track exactly as host tensors of the same frames do: the video stores
    the unnormalised image (a device image would be normalised in place and stored so)."""
    from go_slam_amd.depth_video import DepthVideo
    from go_slam_amd.droid_net import DroidNet
    from go_slam_amd.motion_filter import MotionFilter
    cfg, args = DL.build("tum", parent)
    cfg = {**cfg, "cam": {**cfg["cam"], "H_out": 64, "W_out": 64}}
    torch.manual_seed(3)
    net = DroidNet().to(DEV).eval()

    def run(stream, to_host):
        video = DepthVideo.from_config(_video_cfg(64, 64), types.SimpleNamespace(device=DEV))
        mf = MotionFilter(net, video, thresh=0.0, device=DEV)
        fed = []
        for t, image, depth, intr, pose in stream:
            if to_host:
                image, depth = image.cpu(), depth.cpu()
            fed.append(image.clone())
            mf.track(t, image, depth, intr, gt_pose=pose)
        return video, fed

    v_host, fed = run(D.get_dataset(cfg, args, device=DEV), False)
    v_copy, _ = run(D.get_dataset(cfg, args, device=DEV, output="device"), True)
    n = int(v_host.counter.value)
    assert n >= 1 and n == int(v_copy.counter.value)
    assert torch.equal(v_host.images[:n].cpu(), v_copy.images[:n].cpu())
    assert torch.equal(v_host.images[0].cpu(), fed[0][0])
    v_dev, _ = run(D.get_dataset(cfg, args, device=DEV, output="device"), False)
    assert not torch.equal(v_dev.images[0].cpu(), v_host.images[0].cpu())
