#!/usr/bin/env python
"""Generate tests/golden/datasets.npz by RUNNING THE REFERENCE'S OWN dataset classes (src/datasets.py).

    python tests/golden/gen_golden_datasets.py        # needs the reference tree (as gen_golden.py does)

The folders are tests/dataset_layouts.py's, written to a temporary directory.  cv2 is not installed, so it is replaced
by a stand-in built on PIL and tests/frame_prep_restatement.py: imread decodes with PIL (BGR, grey repeated into three
channels; IMREAD_UNCHANGED as stored), resize / remap / undistort / initUndistortRectifyMap are the restatement's.
numpy 2 removed np.unicode_, which the reference's parse_list names; it is pointed at np.str_.

Recorded per case: the paths relative to the layout's parent, dataset.poses (float64), image_timestamps, and per item
the colour as uint8 levels (the reference's float32 / 255.0 values are level / 255.0f exactly, checked here), depth,
intrinsic and pose."""
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
REF = "/root/reference"
sys.path.insert(0, TESTS)

import dataset_layouts as DL               # noqa: E402
import frame_prep_restatement as R         # noqa: E402


def cv2_standin():
    cv2 = types.ModuleType("cv2")
    cv2.IMREAD_COLOR, cv2.IMREAD_UNCHANGED, cv2.INTER_LINEAR, cv2.CV_32F = 1, -1, 1, 5

    def imread(path, flags=1):
        with Image.open(path) as im:
            if flags == -1:
                return np.array(im)
            return np.ascontiguousarray(np.asarray(im.convert("RGB"))[:, :, ::-1])

    def resize(img, dsize, interpolation=1):
        assert interpolation == 1
        return R.resize_u8(img, dsize[1], dsize[0])

    def remap(img, map_x, map_y, interpolation=1):
        assert interpolation == 1
        return R.remap_u8(img, map_x, map_y)

    def undistort(img, K, D):
        return R.remap_u8(img, *R.undistort_maps(K, D, (img.shape[1], img.shape[0])))

    def initUndistortRectifyMap(K, D, Rm, P, size, m1type):
        assert m1type == 5
        return R.init_undistort_rectify_map(K, D, Rm, P, size)

    cv2.imread, cv2.resize, cv2.remap, cv2.undistort = imread, resize, remap, undistort
    cv2.initUndistortRectifyMap = initUndistortRectifyMap
    return cv2


def load_reference():
    sys.modules["cv2"] = cv2_standin()
    np.unicode_ = np.str_
    spec = importlib.util.spec_from_file_location("ref_datasets", os.path.join(REF, "src", "datasets.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    assert os.path.isdir(REF), "the reference tree is needed to (re)generate the fixtures"
    ref = load_reference()
    out = {}
    with tempfile.TemporaryDirectory() as parent:
        for case in DL.CASES:
            cfg, args = DL.build(case, parent)
            ds = ref.get_dataset(cfg, args, device="cpu")
            rel = lambda ps: np.array([os.path.relpath(p, parent) for p in ps], dtype=np.str_)   # noqa: E731
            out[f"{case}.n_img"] = np.int64(len(ds))
            out[f"{case}.color_paths"] = rel(ds.color_paths)
            if getattr(ds, "right_color_paths", None) is not None:
                out[f"{case}.right_color_paths"] = rel(ds.right_color_paths)
            if ds.depth_paths is not None:
                out[f"{case}.depth_paths"] = rel(ds.depth_paths)
            if ds.poses is not None:
                out[f"{case}.poses"] = np.stack(ds.poses).astype(np.float64)
            if ds.image_timestamps is not None:
                out[f"{case}.image_timestamps"] = np.asarray(ds.image_timestamps, dtype=np.float64)
            levels, depths, intr, poses = [], [], [], []
            for i in range(len(ds)):
                index, color, depth, intrinsic, pose = ds[i]
                assert index == i
                lv = torch.round(color * 255.0).to(torch.uint8)
                assert torch.equal(lv.float() / 255.0, color), case
                levels.append(lv.numpy())
                if depth is not None:
                    depths.append(depth.numpy())
                intr.append(intrinsic.numpy())
                if pose is not None:
                    poses.append(pose.numpy())
            out[f"{case}.color_levels"] = np.stack(levels)
            if depths:
                out[f"{case}.depth"] = np.stack(depths)
            out[f"{case}.intrinsic"] = np.stack(intr)
            if poses:
                out[f"{case}.item_pose"] = np.stack(poses)
    np.savez_compressed(os.path.join(HERE, "datasets.npz"), **out)
    print("wrote datasets.npz", os.path.getsize(os.path.join(HERE, "datasets.npz")), "bytes")
    for k, v in out.items():
        print(" ", k, v.shape, v.dtype)


if __name__ == "__main__":
    main()
