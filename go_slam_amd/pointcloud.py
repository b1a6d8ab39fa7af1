"""The tracked keyframes' coloured dense point cloud, headless (src/visualization.py:104-192, `droid_visualization`).

The reference builds it inside an Open3D window: `iproj` of every dirty keyframe's full-resolution disparity (a
[K, H, W, 3] fp32 intermediate), `depth_filter` against the whole buffer, three masking ops, a copy of everything to the
host and boolean indexing there.  Here csrc/pointcloud.hip filters, compacts and gathers colours in three launches
(count, scan, emit) that write only the surviving points; the one device-to-host read is the per-keyframe offsets,
whose last entry sizes the outputs.  The points, colours, order and per-keyframe slices are the reference sequence's
bit for bit.
"""
import os

import numpy as np
import torch

from . import _lib
from .lietorch_shim import SE3


class PointCloud:
    """points f32 [M, 3] and colors f32 [M, 3] (RGB in [0, 1]) on the device, keyframe `index[b]`'s points in rows
    offsets[b]:offsets[b + 1] (offsets int64 [K + 1] and index int64 [K] on the host)."""

    def __init__(self, points, colors, offsets, index):
        self.points, self.colors = points, colors
        self.offsets, self.index = offsets, index

    def __len__(self):
        return int(self.points.shape[0])

    def keyframe(self, b):
        """(points, colors) of list position b: views into the cloud."""
        lo, hi = int(self.offsets[b]), int(self.offsets[b + 1])
        return self.points[lo:hi], self.colors[lo:hi]

    def numpy(self):
        """(points f32 [M, 3], colors f32 [M, 3]) on the host."""
        return self.points.cpu().numpy(), self.colors.cpu().numpy()

    def export(self, path):
        """Binary little-endian PLY: double x, y, z and uchar red, green, blue per vertex, no face element."""
        write_ply(path, *self.numpy())
        return path


def ply_colors(colors):
    """uchar colours as the reference's writers make them: clamped to [0, 1], times 255, truncated (Open3D's PLY writer
    through rply, and InstantNeuS.extract_color).  The product is taken in double, as Open3D stores colours."""
    return (np.clip(np.asarray(colors, dtype=np.float64), 0.0, 1.0) * 255.0).astype(np.uint8)


def write_ply(path, points, colors):
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    rgb = ply_colors(colors).reshape(-1, 3)
    n = points.shape[0]
    if rgb.shape[0] != n:
        raise ValueError(f"write_ply: {n} points but {rgb.shape[0]} colours")
    rec = np.empty(n, dtype=[("x", "<f8"), ("y", "<f8"), ("z", "<f8"),
                             ("red", "u1"), ("green", "u1"), ("blue", "u1")])
    rec["x"], rec["y"], rec["z"] = points[:, 0], points[:, 1], points[:, 2]
    rec["red"], rec["green"], rec["blue"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    header = ("ply\nformat binary_little_endian 1.0\n"
              f"element vertex {n}\n"
              "property double x\nproperty double y\nproperty double z\n"
              "property uchar red\nproperty uchar green\nproperty uchar blue\n"
              "end_header\n")
    with open(path, "wb") as fh:
        fh.write(header.encode("ascii"))
        fh.write(rec.tobytes())


def _host_index(index, n):
    """int64 host tensor of the listed keyframes; each must lie in [0, n)."""
    idx = torch.as_tensor(index).reshape(-1).to(device="cpu", dtype=torch.int64)
    if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= n):
        raise IndexError(f"keyframe_point_cloud: index outside [0, {n})")
    return idx


def _rows(buf, idx):
    """buf[idx] as torch.index_select makes it; a contiguous run of whole rows is taken as a view when every row starts
    16-byte aligned (the reduction then sees the same rows at the same alignment as in a fresh copy)."""
    k = idx.numel()
    a = int(idx[0])
    hw = buf[0].numel()
    if buf.is_contiguous() and hw % 4 == 0 and bool(torch.equal(idx, torch.arange(a, a + k))):
        return buf[a:a + k]
    return torch.index_select(buf, 0, idx.to(buf.device))


def _empty(device):
    z = torch.empty(0, 3, dtype=torch.float32, device=device)
    return PointCloud(z, z.clone(), torch.zeros(1, dtype=torch.int64), torch.zeros(0, dtype=torch.int64))


@torch.no_grad()
def keyframe_point_cloud(video, index=None, filter_thresh=0.01, visible_num=2, source="tracked"):
    """The coloured point cloud of keyframes `index` (default: every keyframe below `video.counter`) of a full-resolution
    DepthVideo, as PointCloud.

    source="tracked": the reference viewer's cloud (src/visualization.py:116-150).  Points are iproj of `disps_up`
    through SE3(poses[index]).inv() at intrinsics[0] * 8; a pixel is kept when depth_filter over the WHOLE buffers
    (every slot a possible neighbour, stale ones past the counter included) counts at least `visible_num` consistent
    views at `filter_thresh`, and its disparity exceeds 0.01 x its keyframe's mean disparity.
    source="filtered": the cloud MultiviewFilter handed to the mapper, keyframes [0, filtered_id): iproj of
    `disps_filtered` through w2w * SE3(poses_filtered).inv(), kept where `mask_filtered` is non-zero (`index` must be
    None).  Colours are `images[ix]` at the pixel in both."""
    disps_up = video.disps_up
    dev = disps_up.device
    num, H, W = disps_up.shape
    if source == "tracked":
        idx = _host_index(range(int(video.counter.value)) if index is None else index, num)
    elif source == "filtered":
        if index is not None:
            raise ValueError("keyframe_point_cloud: source='filtered' covers [0, filtered_id); index must be None")
        idx = torch.arange(max(int(video.filtered_id[0].item()), 0), dtype=torch.int64)
    else:
        raise ValueError(f"keyframe_point_cloud: unknown source {source!r}")
    k = idx.numel()
    if k == 0:
        return _empty(dev)
    L = _lib.lib()
    ws_bytes = L.gs_pointcloud_workspace_bytes(k, H, W)
    if ws_bytes == 0:
        raise ValueError(f"keyframe_point_cloud: unsupported shape k={k}, {H} x {W}")
    with torch.cuda.device(dev):
        st = _lib.stream_ptr(dev)
        index_d = idx.to(dev)
        intr = (video.intrinsics[0] * 8).contiguous()
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        if source == "tracked":
            disps = disps_up
            poses_inv = SE3(video.poses[index_d]).inv().data.contiguous()
            floor = (0.01 * _rows(disps_up, idx).mean(dim=[1, 2])).contiguous()
            rc = L.gs_pointcloud_count(_lib.ptr(video.poses), _lib.ptr(disps_up), _lib.ptr(intr), _lib.ptr(index_d),
                                       _lib.ptr(floor), float(filter_thresh), float(visible_num), k, num, H, W,
                                       _lib.ptr(ws), ws_bytes, st)
            _lib.check(rc, "keyframe_point_cloud: count")
        else:
            disps = video.disps_filtered
            w2w = SE3(video.pose_compensate[0].clone().unsqueeze(0))
            poses_inv = (w2w * SE3(video.poses_filtered[:k]).inv()).data.contiguous()
            rc = L.gs_pointcloud_mask(_lib.ptr(video.mask_filtered), _lib.ptr(index_d), k, num, H, W, _lib.ptr(ws),
                                      ws_bytes, st)
            _lib.check(rc, "keyframe_point_cloud: mask")
        offsets = torch.empty(k + 1, dtype=torch.int64, device=dev)
        _lib.check(L.gs_pointcloud_scan(k, H, W, _lib.ptr(ws), ws_bytes, _lib.ptr(offsets), st),
                   "keyframe_point_cloud: scan")
        offsets = offsets.cpu()
        m = int(offsets[k])
        points = torch.empty(m, 3, dtype=torch.float32, device=dev)
        colors = torch.empty(m, 3, dtype=torch.float32, device=dev)
        rc = L.gs_pointcloud_emit(_lib.ptr(poses_inv), _lib.ptr(disps), _lib.ptr(intr), _lib.ptr(video.images),
                                  _lib.ptr(index_d), k, num, H, W, _lib.ptr(ws), ws_bytes, m, _lib.ptr(points),
                                  _lib.ptr(colors), st)
        _lib.check(rc, "keyframe_point_cloud: emit")
    return PointCloud(points, colors, offsets, idx)


class PointCloudExporter:
    """The headless counterpart of droid_visualization's state (src/visualization.py:55-192): per keyframe its slice of
    the cloud, refreshed from `video.dirty`, and the keyboard's filter controls."""

    def __init__(self, video, save_root, device=None, filter_thresh=0.01, visible_num=2):
        self.video = video
        self.device = torch.device(device) if device is not None else video.disps_up.device
        self.filter_thresh = filter_thresh
        self.visible_num = visible_num
        self.points = {}                 # keyframe index -> (points, colors) on the device
        self.last_id = -1
        self.out_dir = os.path.join(save_root, "pointcloud")
        os.makedirs(self.out_dir, exist_ok=True)

    @torch.no_grad()
    def update(self):
        """Recompute the dirty keyframes, replace their slices, clear their flags (animation_callback, :108-150: the
        flags are read under the video lock and cleared after it).  Returns how many keyframes were refreshed."""
        v = self.video
        with v.get_lock():
            dirty_index, = torch.where(v.dirty.clone())
        if len(dirty_index) == 0:
            return 0
        v.dirty[dirty_index] = False
        cloud = keyframe_point_cloud(v, dirty_index, self.filter_thresh, self.visible_num)
        for b, ix in enumerate(cloud.index.tolist()):
            self.points[ix] = cloud.keyframe(b)
        return len(cloud.index)

    def _redirty(self):
        v = self.video
        with v.get_lock():
            v.dirty[:v.counter.value] = True

    def increase_filter(self):
        self.filter_thresh *= 2
        self._redirty()

    def decrease_filter(self):
        self.filter_thresh *= 1 / 2
        self._redirty()

    def cloud(self):
        """Every stored keyframe's slice, concatenated in ascending keyframe order."""
        keys = sorted(self.points)
        if not keys:
            return _empty(self.device)
        pts = [self.points[i][0] for i in keys]
        sizes = torch.tensor([0] + [p.shape[0] for p in pts], dtype=torch.int64)
        return PointCloud(torch.cat(pts), torch.cat([self.points[i][1] for i in keys]), torch.cumsum(sizes, 0),
                          torch.tensor(keys, dtype=torch.int64))

    def save_id(self):
        """save_pointcloud's file number (:86-95): the largest position in range(len(points)), i.e. one less than the
        number of stored keyframes."""
        return len(self.points) - 1

    def save(self):
        """{save_root}/pointcloud/{id:05d}_pc.ply of cloud(); remembers id as the last saved one."""
        self.last_id = self.save_id()
        return self.cloud().export(os.path.join(self.out_dir, f"{self.last_id:05d}_pc.ply"))
