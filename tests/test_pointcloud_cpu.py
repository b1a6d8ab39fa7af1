"""Keyframe point cloud without a GPU: the restatement on a hand-worked case, the PLY layout and the save rules."""
import contextlib
import os
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from go_slam_amd import pointcloud as PC          # noqa: E402
from go_slam_amd import visualization as VIS      # noqa: E402
from go_slam_amd.neus.mesh import load_mesh       # noqa: E402
import pointcloud_restatement as R                # noqa: E402

HT, WD = 3, 4


def hand_case():
    """Six slots of 3 x 4 pixels at identity poses with fx = fy = 1, cx = cy = 0, so that every pixel projects onto
    itself in every other slot and its four taps are (v, u), (v, u+1), (v+1, u), (v+1, u+1).  Keyframes 0-2 are
    listed; slots 3-5 are past the counter but still count as neighbours."""
    poses = torch.zeros(6, 7)
    poses[:, 6] = 1.0
    disps = torch.ones(6, HT, WD)
    disps[2] = 0.5                    # depth 2: exactly 1 from depth 1
    disps[4] = 0.5
    disps[5] = 0.0                    # 1 / 0 = inf: never consistent
    disps[0, 1, 1] = 0.001            # below 0.01 x mean, yet consistent with slot 3 ...
    disps[3, 1, 1] = 0.001            # ... which holds the same depth there
    images = torch.rand(6, 3, HT, WD, generator=torch.Generator().manual_seed(0))
    intr = torch.tensor([1.0, 1.0, 0.0, 0.0])
    return poses, disps, images, intr


def test_restatement_counts_by_hand():
    poses, disps, images, intr = hand_case()
    inner = torch.zeros(HT, WD)
    inner[:HT - 1, :WD - 1] = 1.0     # u0 < wd-1 and v0 < ht-1: the last row and column never count
    count = R.tracked_counts(poses, disps, intr, [0, 1, 2], 0.1)
    # keyframe 0: neighbours 3 (same depths) 4 (depth 2) 5 (zero) -> 1; keyframe 1: 0 (its tap (1,1) misses, (1,2)
    # hits: the else-if chain) 4 5 -> 1; keyframe 2: 1 0 5, all a full unit of depth away -> 0
    assert torch.equal(count, torch.stack([inner, inner, 0 * inner]))
    # an inverse-depth difference of exactly thresh is not consistent (strict <); one float step above it is
    assert torch.equal(R.tracked_counts(poses, disps, intr, [2], 1.0)[0], 0 * inner)
    above = float(np.nextafter(np.float32(1.0), np.float32(2.0)))
    assert torch.equal(R.tracked_counts(poses, disps, intr, [2], above)[0], 2 * inner)


def test_restatement_cloud_by_hand():
    poses, disps, images, intr = hand_case()
    pts, clr, offsets = R.tracked_cloud(poses, disps, images, intr, [0, 1, 2], thresh=0.1, visible_num=1)
    keep = [(0, v, u) for v in range(HT - 1) for u in range(WD - 1) if (v, u) != (1, 1)]
    keep += [(1, v, u) for v in range(HT - 1) for u in range(WD - 1)]
    assert offsets.tolist() == [0, 5, 11, 11]
    # identity pose, unit intrinsics: (u, v, 1) / d
    want = torch.tensor([[u / disps[k, v, u], v / disps[k, v, u], 1 / disps[k, v, u]] for k, v, u in keep])
    assert torch.equal(pts, want)
    assert torch.equal(clr, torch.stack([images[k, :, v, u] for k, v, u in keep]))
    # visible_num 2 keeps nothing, and an empty selection is an empty cloud
    pts2, _, off2 = R.tracked_cloud(poses, disps, images, intr, [0, 1, 2], thresh=0.1, visible_num=2)
    assert pts2.shape == (0, 3) and off2.tolist() == [0, 0, 0, 0]


def test_ply_layout_and_round_trip(tmp_path):
    pts = np.array([[0.0, 1.0, 2.0], [-1.5, 1e-7, 3e5], [0.25, 0.5, 0.75], [1, 2, 3], [4, 5, 6]])
    rgb = np.array([[0.0, 1.0, 0.5], [-0.2, 1.7, 0.999], [0.5, 0.5, 0.5], [1.0, 0.0, 0.0], [0.1, 0.2, 0.3]],
                   dtype=np.float32)
    path = str(tmp_path / "c.ply")
    cloud = PC.PointCloud(torch.tensor(pts, dtype=torch.float32), torch.tensor(rgb), torch.tensor([0, 5]),
                          torch.tensor([0]))
    cloud.export(path)
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    assert head.decode().splitlines() == [
        "ply", "format binary_little_endian 1.0", "element vertex 5",
        "property double x", "property double y", "property double z",
        "property uchar red", "property uchar green", "property uchar blue"]
    assert b"face" not in head
    assert len(body) == 5 * (3 * 8 + 3)
    m = load_mesh(path)
    assert np.array_equal(m.vertices, pts.astype(np.float32).astype(np.float64))
    assert m.faces.shape == (0, 3)
    assert m.vertex_colors.tolist() == [[0, 255, 127], [0, 255, 254], [127, 127, 127], [255, 0, 0], [25, 51, 76]]


def _fake_video(n_slots):
    v = types.SimpleNamespace()
    v.dirty = torch.zeros(n_slots, dtype=torch.bool)
    v.counter = types.SimpleNamespace(value=0)
    v.disps_up = torch.zeros(n_slots, 1, 1)
    v.get_lock = contextlib.nullcontext
    return v


def _fake_cloud(video, index, filter_thresh=0.01, visible_num=2):
    """two points per keyframe, x = keyframe index"""
    idx = torch.as_tensor(index).reshape(-1).cpu()
    pts = torch.stack([idx.float().repeat_interleave(2), torch.zeros(2 * len(idx)), torch.ones(2 * len(idx))], 1)
    return PC.PointCloud(pts, torch.full_like(pts, 0.5), torch.arange(0, 2 * len(idx) + 1, 2), idx)


def test_save_names_and_every_25_keyframes(tmp_path, monkeypatch):
    monkeypatch.setattr(PC, "keyframe_point_cloud", _fake_cloud)
    monkeypatch.setattr(VIS.droid_visualization, "exporter", None)
    video = _fake_video(80)
    root = str(tmp_path)
    saved = []
    for n in range(1, 61):        # one new keyframe per tick; every fifth one is only marked dirty at the next tick
        video.counter.value = n
        if n % 5 != 0:
            video.dirty[n - 1] = True
            if n % 5 == 1 and n > 1:
                video.dirty[n - 2] = True
        before = set(os.listdir(os.path.join(root, "pointcloud"))) if n > 1 else set()
        refreshed = VIS.droid_visualization(video, device="cpu", save_root=root)
        assert refreshed == (0 if n % 5 == 0 else 1 + int(n % 5 == 1 and n > 1))
        assert not bool(video.dirty.any())
        saved += [(n, f) for f in sorted(set(os.listdir(os.path.join(root, "pointcloud"))) - before)]
    ex = VIS.droid_visualization.exporter
    # the id is one less than the number of stored keyframes; a file once it is more than 25 past the last one (-1)
    assert saved == [(26, "00025_pc.ply"), (52, "00051_pc.ply")]
    assert ex.last_id == 51 and len(ex.points) == 59
    m = load_mesh(os.path.join(root, "pointcloud", "00051_pc.ply"))
    assert m.vertices[:, 0].tolist() == [float(i) for i in range(52) for _ in range(2)]
    # increase / decrease re-dirty [:counter] and scale the threshold
    VIS.droid_visualization.increase_filter()
    assert ex.filter_thresh == 0.02 and int(video.dirty.sum()) == 60
    video.dirty[:] = False
    VIS.droid_visualization.decrease_filter()
    assert ex.filter_thresh == 0.01 and int(video.dirty.sum()) == 60


def test_exporter_save_writes_cloud_in_index_order(tmp_path):
    ex = PC.PointCloudExporter(_fake_video(8), str(tmp_path), device="cpu")
    for ix in (4, 0, 2):
        c = _fake_cloud(None, [ix])
        ex.points[ix] = c.keyframe(0)
    path = ex.save()
    assert os.path.basename(path) == "00002_pc.ply" and ex.last_id == 2
    cloud = ex.cloud()
    assert cloud.index.tolist() == [0, 2, 4] and cloud.offsets.tolist() == [0, 2, 4, 6]
    m = load_mesh(path)
    assert np.array_equal(m.vertices, cloud.points.double().numpy())
    assert (m.vertex_colors == 127).all()


def test_bad_arguments_are_refused():
    video = types.SimpleNamespace(disps_up=torch.zeros(4, 2, 2), counter=types.SimpleNamespace(value=2))
    with pytest.raises(IndexError):
        PC.keyframe_point_cloud(video, [0, 4])
    with pytest.raises(ValueError):
        PC.keyframe_point_cloud(video, [0], source="filtered")
    with pytest.raises(ValueError):
        PC.keyframe_point_cloud(video, source="mapped")
