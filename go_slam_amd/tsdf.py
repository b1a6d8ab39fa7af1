"""Surfaces without the mapper: keyframe depth fused into a truncated signed distance volume and meshed on the GPU.

The reference has no such path -- under `only_tracking` it ends with a trajectory and a point cloud.  Here
csrc/tsdf.hip integrates depth maps at given world-to-camera poses into a dense lattice (one lane per lattice point, a
batch of frames per launch, no atomics), `neus.mesh.marching_cubes` meshes it, and a second kernel drops the vertices
next to never-observed points and colours the rest.  Arithmetic contract: include/goslam_hip.h (gs_tsdf_*);
tests/tsdf_restatement.py restates it serially.
"""
import math
import os

import numpy as np
import torch

from . import _lib
from .lietorch_shim import SE3
from .neus.mesh import Mesh, marching_cubes
from .pointcloud import _host_index, _rows, ply_colors

MAX_POINTS = 1024          # per axis: marching_cubes' limit
CHUNK = 32                 # keyframes converted from inverse depth at a time in fuse_keyframes


def w2c_matrices(w2c):
    """float32 [K,3,4] world-to-camera matrices from [K,7] (t, q) vectors as `video.poses` stores them, or from
    [K,4,4] / [K,3,4] matrices.  Quaternions are expanded in float64 on the tensor's device and rounded once."""
    w2c = torch.as_tensor(w2c)
    if w2c.dim() == 2 and w2c.shape[1] == 7:
        m = SE3(w2c.double()).matrix()[:, :3, :]
    elif w2c.dim() == 3 and tuple(w2c.shape[1:]) in ((4, 4), (3, 4)):
        m = w2c[:, :3, :]
    else:
        raise ValueError(f"w2c must be [K,7], [K,4,4] or [K,3,4] (got {tuple(w2c.shape)})")
    return m.to(torch.float32).contiguous()


class TSDFVolume:
    """A dense TSDF over `bound` ([3,2]: lo, hi per axis) with lattice points at lo + idx * voxel_size,
    n = ceil((hi - lo) / voxel_size) + 1 per axis.  `.tsdf` (+1 where nothing was seen) and `.weight` are float32
    [nx,ny,nz], `.colors` float32 [3,nx,ny,nz], on `device`."""

    def __init__(self, bound, voxel_size, trunc=None, max_weight=64.0, device=None):
        bound = np.asarray(bound.detach().cpu() if isinstance(bound, torch.Tensor) else bound, dtype=np.float64)
        if bound.shape != (3, 2):
            raise ValueError(f"TSDFVolume: bound must be [3,2] (got {bound.shape})")
        self.voxel = float(voxel_size)
        if not self.voxel > 0:
            raise ValueError(f"TSDFVolume: voxel_size must be positive (got {voxel_size})")
        self.lo = bound[:, 0].copy()
        dims = []
        for axis, name in enumerate("xyz"):
            n = int(math.ceil((bound[axis, 1] - bound[axis, 0]) / self.voxel)) + 1
            if n > MAX_POINTS:
                raise ValueError(f"TSDFVolume: axis {name} needs {n} lattice points at voxel_size {self.voxel} "
                                 f"(at most {MAX_POINTS}); enlarge voxel_size or shrink the bound")
            if n < 2:
                raise ValueError(f"TSDFVolume: axis {name} of the bound is empty")
            dims.append(n)
        self.dims = tuple(dims)
        self.trunc = 4.0 * self.voxel if trunc is None else float(trunc)
        self.max_weight = float(max_weight)
        if not self.trunc > 0 or not self.max_weight >= 1:
            raise ValueError(f"TSDFVolume: trunc {self.trunc} must be positive and max_weight {self.max_weight} >= 1")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.tsdf = torch.empty(self.dims, dtype=torch.float32, device=self.device)
        self.weight = torch.empty(self.dims, dtype=torch.float32, device=self.device)
        self.colors = torch.empty((3,) + self.dims, dtype=torch.float32, device=self.device)
        self.reset()

    def reset(self):
        self.tsdf.fill_(1.0)
        self.weight.zero_()
        self.colors.zero_()

    @torch.no_grad()
    def integrate(self, depth, w2c, intrinsics, images=None, mask=None):
        """Fuse K frames in order: depth [K,H,W] in metres (<= 0 invalid), w2c [K,7] / [K,4,4] / [K,3,4],
        intrinsics (fx, fy, cx, cy) of the depth maps, images [K,3,H,W] in [0,1] and mask [K,H,W] (0 drops a pixel)
        optional.  Enqueues ceil(K / batch) launches on the current stream; nothing is read back."""
        dev = self.device

        def f32(t, what, shape):
            t = torch.as_tensor(t).to(device=dev, dtype=torch.float32).contiguous()
            if tuple(t.shape) != shape:
                raise ValueError(f"TSDFVolume.integrate: {what} must be {list(shape)} (got {list(t.shape)})")
            return t

        depth = torch.as_tensor(depth)
        if depth.dim() != 3:
            raise ValueError(f"TSDFVolume.integrate: depth must be [K,H,W] (got {list(depth.shape)})")
        K, H, W = (int(s) for s in depth.shape)
        depth = f32(depth, "depth", (K, H, W))
        mats = w2c_matrices(w2c).to(dev)
        if mats.shape[0] != K:
            raise ValueError(f"TSDFVolume.integrate: {mats.shape[0]} poses for {K} depth maps")
        images = None if images is None else f32(images, "images", (K, 3, H, W))
        mask = None if mask is None else f32(mask, "mask", (K, H, W))
        intr = torch.as_tensor(intrinsics).detach().cpu().reshape(-1).tolist() if not isinstance(intrinsics, (tuple, list)) \
            else list(intrinsics)
        if len(intr) != 4:
            raise ValueError("TSDFVolume.integrate: intrinsics must be (fx, fy, cx, cy)")
        if K == 0:
            return self
        nx, ny, nz = self.dims
        with torch.cuda.device(dev):
            rc = _lib.lib().gs_tsdf_integrate(
                _lib.ptr(self.tsdf), _lib.ptr(self.weight), _lib.ptr(self.colors), nx, ny, nz, _lib.ptr(depth),
                _lib.ptr(mask), _lib.ptr(images), _lib.ptr(mats), K, H, W, *[float(v) for v in intr],
                float(self.lo[0]), float(self.lo[1]), float(self.lo[2]), self.voxel, self.trunc, self.max_weight,
                _lib.stream_ptr(dev))
        _lib.check(rc, "TSDFVolume.integrate")
        return self

    @torch.no_grad()
    def vertex_attr(self, verts, min_weight=1.0):
        """(keep bool [V], rgb float32 [V,3]) of marching-cubes vertices in index space (gs_tsdf_vertex_attr)."""
        verts = verts.to(device=self.device, dtype=torch.float32).contiguous()
        V = int(verts.shape[0])
        keep = torch.empty(V, dtype=torch.uint8, device=self.device)
        rgb = torch.empty(V, 3, dtype=torch.float32, device=self.device)
        nx, ny, nz = self.dims
        with torch.cuda.device(self.device):
            rc = _lib.lib().gs_tsdf_vertex_attr(_lib.ptr(verts), V, _lib.ptr(self.weight), _lib.ptr(self.colors), nx,
                                                ny, nz, float(min_weight), _lib.ptr(keep), _lib.ptr(rgb),
                                                _lib.stream_ptr(self.device))
        _lib.check(rc, "TSDFVolume.vertex_attr")
        return keep.bool(), rgb

    @torch.no_grad()
    def extract_mesh(self, min_weight=1.0):
        """The zero level as a `Mesh` in world coordinates with uint8 vertex colours, normals toward free space.  Faces
        with a vertex on an edge whose endpoints were seen fewer than `min_weight` times are dropped: that is the sheet
        between observed space behind a surface and never-observed space."""
        with torch.cuda.device(self.device):
            verts, faces = marching_cubes(-self.tsdf, 0.0)
            if faces.shape[0] == 0:
                return Mesh(np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int64), np.zeros((0, 3), dtype=np.uint8))
            keep, rgb = self.vertex_attr(verts, min_weight)
            face_keep = keep[faces.long()].all(dim=1)
        mesh = Mesh(verts.cpu().numpy(), faces.cpu().numpy(), ply_colors(rgb.cpu().numpy()))
        mesh.update_faces(face_keep)
        mesh.remove_unreferenced_vertices()
        mesh.vertices = np.ascontiguousarray(mesh.vertices * self.voxel + self.lo[None, :])
        return mesh


def _inverse(disp):
    return torch.where(disp > 0, 1.0 / disp, torch.zeros_like(disp))


@torch.no_grad()
def fuse_keyframes(video, bound, voxel_size, source="tracked", index=None, trunc=None, filter_thresh=0.01, visible_num=2,
                   min_weight=1.0):
    """Fuse keyframes of a full-resolution DepthVideo into a TSDFVolume over `bound` and mesh it: (TSDFVolume, Mesh).

    Every pose is composed with `video.pose_compensate[0]` (camera-to-world = w2w * SE3(pose).inv(), as
    keyframe_point_cloud(source="filtered") and Mesher.update_param_from_mapping do), so the mesh is in the frame of
    est_poses.npy and of the NeuS mesh.
    source="tracked": depth 1 / disps_up of keyframes `index` (default: all below the counter), masked by
    keyframe_point_cloud(source="tracked")'s rule: depth_filter count over the whole buffers >= visible_num at
    filter_thresh, and disparity > 0.01 x the keyframe's mean.
    source="filtered": disps_filtered, mask_filtered and poses_filtered of keyframes [0, filtered_id); index must be None.
    source="sensor": depths_gt at the tracked poses, unmasked; needs rgbd mode."""
    from . import droid_backends
    dev = video.disps_up.device
    num = int(video.disps_up.shape[0])
    if source in ("tracked", "sensor"):
        if source == "sensor" and getattr(video, "cfg", None) is not None and video.cfg.get("mode", "rgbd") != "rgbd":
            raise ValueError(f"fuse_keyframes: source='sensor' needs rgbd mode (mode is {video.cfg.get('mode')!r}: "
                             "no sensor depth is stored)")
        idx = _host_index(range(int(video.counter.value)) if index is None else index, num)
    elif source == "filtered":
        if index is not None:
            raise ValueError("fuse_keyframes: source='filtered' covers [0, filtered_id); index must be None")
        idx = torch.arange(max(int(video.filtered_id[0].item()), 0), dtype=torch.int64)
    else:
        raise ValueError(f"fuse_keyframes: unknown source {source!r}")
    vol = TSDFVolume(bound, voxel_size, trunc=trunc, device=dev)
    intr = (video.intrinsics[0] * 8).contiguous()
    intr_host = intr.cpu().tolist()
    w2w_inv = SE3(video.pose_compensate[0].clone().unsqueeze(0)).inv()
    poses = video.poses_filtered if source == "filtered" else video.poses
    for a in range(0, idx.numel(), CHUNK):
        ids = idx[a:a + CHUNK]
        ids_d = ids.to(dev)
        w2c = (SE3(poses[ids_d]) * w2w_inv).data       # the inverse of w2w * SE3(pose).inv(); exact for the identity
        mask = None
        if source == "tracked":
            disps = _rows(video.disps_up, ids)
            thresh = float(filter_thresh) * torch.ones(ids.numel(), dtype=torch.float32, device=dev)
            count = droid_backends.depth_filter(video.poses, video.disps_up, intr, ids_d, thresh)
            mask = ((count >= visible_num) & (disps > 0.01 * disps.mean(dim=[1, 2], keepdim=True))).float()
            depth = _inverse(disps)
        elif source == "filtered":
            depth = _inverse(_rows(video.disps_filtered, ids))
            mask = _rows(video.mask_filtered, ids)
        else:
            depth = _rows(video.depths_gt, ids)
        vol.integrate(depth, w2c, intr_host, images=_rows(video.images, ids), mask=mask)
    return vol, vol.extract_mesh(min_weight)


def fuse_from_config(slam, stream=None, trans_init=None):
    """`SLAM.terminate`'s TSDF step: with cfg["tsdf"]["enable"], fuse the run's keyframes, write
    {output}/mesh/tsdf_mesh.ply and, with a readable meshing.gt_mesh_path and meshing.eval_rec, align and evaluate it
    into {output}/metrics_tsdf_mesh.txt.  Returns the Mesh, or None when the key is absent or disabled."""
    opt = slam.cfg.get("tsdf") or {}
    if not opt.get("enable", False):
        return None
    bound = opt.get("bound") or slam.cfg["mapping"]["bound"]
    _, mesh = fuse_keyframes(slam.video, bound, float(opt.get("voxel_size", 0.05)), source=opt.get("source", "tracked"),
                             trunc=opt.get("truncation"), min_weight=float(opt.get("min_weight", 1.0)))
    os.makedirs(f"{slam.output}/mesh", exist_ok=True)
    mesh.export(f"{slam.output}/mesh/tsdf_mesh.ply")
    meshing = slam.cfg.get("meshing") or {}
    gt_path = meshing.get("gt_mesh_path") or ""
    if meshing.get("eval_rec") and gt_path.find(".ply") > -1 and os.path.exists(gt_path) and len(mesh.faces) > 0:
        from .neus.mesh import load_mesh
        from .neus.mesh_eval import align_mesh, eval_mesh
        gt_mesh = load_mesh(gt_path)
        aligned = align_mesh(mesh.copy(), gt_mesh, threshold=0.1, trans_init=trans_init)
        eval_mesh(aligned, gt_mesh, N3d=meshing.get("n_points_to_eval", 200000),
                  dist_th=meshing.get("mesh_threshold_to_eval", 0.05), out_path=f"{slam.output}/metrics_tsdf_mesh.txt")
    return mesh
