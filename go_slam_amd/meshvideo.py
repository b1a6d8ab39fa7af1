"""Headless drop-in for src/tools/meshvideo.py's `MeshVideo`: the reconstruction video -- the growing
mesh, the estimated and ground-truth camera frusta and the two trajectories -- rendered on the GPU, without Open3D, a
window or a child process.

- `render_mesh_frames`: colour frames of a mesh with depth-tested line overlays at many poses: a visibility buffer
  (gs_mesh_visbuf, gs_line_visbuf), area-weighted vertex normals (gs_vertex_normals) and a resolve pass
  (gs_visbuf_resolve).  Contracts: include/goslam_neus.h; tests/meshvideo_restatement.py restates them on the CPU.
- `MeshVideo`: the reference's class.  Every `update_*` / `reset` call is one tick of the reference's animation callback:
  it applies the message, renders one frame and, with `save_rendering`, writes
  `{output}/tmp_rendering/{frame_idx:06d}.jpg`.

Deliberate differences from the reference: our own shading (a two-sided headlight on vertex colours) instead
of Open3D's GL pipeline; no back-face culling; one-pixel lines without anti-aliasing; a frame per message instead of a
frame per window refresh.
"""
import math
import os
import shutil
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from .neus.mesh import Mesh, load_mesh
from .neus.mesher import ZNEAR, _as_tensor, _c2w_tensor, _device

GT_COLOR = (0.0, 1.0, 0.0)       # ground truth: green
EST_COLOR = (0.0, 0.0, 1.0)      # estimates (keyframes too): blue
ZFAR = 1000.0                    # the reference's set_constant_z_far
GT_ID_OFFSET = int(1e8)          # ground-truth cameras live beside the estimates in one table

# the camera actor: the image-plane rectangle at z = 1.5 with its diagonals, the four rays from the centre, and a
# triangle marking the up side
CAM_POINTS = np.array([[0, 0, 0], [-1, -1, 1.5], [1, -1, 1.5], [1, 1, 1.5], [-1, 1, 1.5], [-0.5, 1, 1.5], [0.5, 1, 1.5],
                       [0, 1.2, 1.5]], dtype=np.float64)
CAM_LINES = np.array([[1, 2], [2, 3], [3, 4], [1, 4], [1, 3], [2, 4], [0, 1], [0, 2], [0, 3], [0, 4], [5, 7], [6, 7]],
                     dtype=np.int64)

DeviceMesh = namedtuple("DeviceMesh", "vertices faces colors normals")


def camera_actor(is_gt=False, is_keyframe=False, scale=1e-3):
    """The reference's create_camera_actor as arrays: points float64 [8,3], segments int64 [12,2], colours float64
    [12,3].  Keyframes are drawn at a seventh of the scale."""
    if is_keyframe:
        scale = scale / 7
    color = GT_COLOR if is_gt else EST_COLOR
    return scale * CAM_POINTS, CAM_LINES.copy(), np.tile(np.asarray(color, np.float64), (len(CAM_LINES), 1))


def transform_points(points, matrix):
    """Open3D's Geometry3D.transform on points [N,3]: M [p, 1], divided by the homogeneous coordinate."""
    M = np.asarray(matrix, np.float64)
    h = np.concatenate([points, np.ones((len(points), 1))], 1) @ M.T
    return h[:, :3] / h[:, 3:]


def trajectory_actor(c2w_list, i, is_gt):
    """The reference's trajectory line set: the camera centres c2w_list[1:i, :3, 3], consecutive ones joined."""
    pts = c2w_list[1:i, :3, 3]
    pts = pts.detach().cpu().numpy() if isinstance(pts, torch.Tensor) else np.asarray(pts)
    pts = pts.astype(np.float64).reshape(-1, 3)
    n = max(len(pts) - 1, 0)
    lines = np.stack([np.arange(n), np.arange(n) + 1], 1).astype(np.int64).reshape(-1, 2)
    return pts, lines, np.tile(np.asarray(GT_COLOR if is_gt else EST_COLOR, np.float64), (n, 1))


def viewer_extrinsic(init_pose):
    """The world-to-camera matrix the reference hands to the view control: `init_pose` (camera-to-world) moved 2 along
    its z column's direction, its y and z columns negated, inverted.  `init_pose` is modified in place, as there."""
    init_pose[:3, 3] += 2 * (init_pose[:3, 2] / np.linalg.norm(init_pose[:3, 2]))
    init_pose[:3, 2] *= -1
    init_pose[:3, 1] *= -1
    return np.linalg.inv(init_pose)


def default_intrinsics(H, W, fov_y_deg=60.0):
    """(fx, fy, cx, cy) of a pinhole camera with a `fov_y_deg` vertical field of view, square pixels and the principal
    point at (W/2 - 0.5, H/2 - 0.5)."""
    f = 0.5 * H / math.tan(math.radians(0.5 * fov_y_deg))
    return f, f, W / 2 - 0.5, H / 2 - 0.5


def normal_scale(vertices, n_faces):
    """The fixed-point scale of gs_vertex_normals: the largest power of two with scale * extent^2 * F <= 2^62 (extent =
    the diagonal of the finite vertices' bounding box), so that no vertex' sum can overflow whatever its valence."""
    v = vertices[torch.isfinite(vertices).all(1)]
    extent = float(torch.linalg.norm((v.max(0).values - v.min(0).values).double())) if v.shape[0] else 0.0
    bound = max(extent * extent, 1e-200) * max(int(n_faces), 1)
    return 2.0 ** min(math.floor(62 - math.log2(bound)), 900)


def vertex_normals(vertices, faces, device=None, return_sums=False):
    """Area-weighted unit vertex normals, a device float32 [V,3] (zero where a vertex has no face with area); bitwise
    reproducible.  `return_sums` also returns the fixed-point sums int64 [V,3] and their scale."""
    dev = _device(device)
    v, f = _as_tensor(vertices, torch.float32, dev), _as_tensor(faces, torch.int32, dev)
    sums = torch.empty(v.shape[0], 3, dtype=torch.int64, device=dev)
    normals = torch.empty(v.shape[0], 3, dtype=torch.float32, device=dev)
    scale = normal_scale(v, f.shape[0])
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().gs_vertex_normals(_lib.ptr(v), v.shape[0], _lib.ptr(f), f.shape[0], scale, _lib.ptr(sums),
                                                _lib.ptr(normals), _lib.stream_ptr(dev)), "vertex_normals")
    return (normals, sums, scale) if return_sums else normals


def upload_mesh(mesh, device=None):
    """A mesh on the device, ready to be drawn many times: `mesh` is None (nothing), a Mesh, or (vertices, faces[, uint8
    vertex colours]); the vertex normals are computed here."""
    if isinstance(mesh, DeviceMesh):
        return mesh
    dev = _device(device)
    if mesh is None:
        mesh = (np.zeros((0, 3)), np.zeros((0, 3), np.int64))
    if isinstance(mesh, Mesh):
        v, f, c = mesh.vertices, mesh.faces, mesh.vertex_colors
    else:
        v, f, c = (tuple(mesh) + (None,))[:3]
    v, f = _as_tensor(v, torch.float32, dev), _as_tensor(f, torch.int32, dev)
    if c is not None:
        c = _as_tensor(c, torch.uint8, dev).reshape(-1, 3)
        if c.shape[0] != v.shape[0]:
            raise ValueError(f"upload_mesh: {c.shape[0]} vertex colours for {v.shape[0]} vertices")
    return DeviceMesh(v, f, c, vertex_normals(v, f, dev))


def world_to_camera(c2w, device):
    """w2c float32 [K,3,4] of camera-to-world matrices [K,4,4]: inverted in float64, rounded once."""
    return torch.linalg.inv(c2w.to(device=device, dtype=torch.float64))[:, :3, :].float().contiguous()


def _pack_rgb(rgb):
    r, g, b = (int(x) for x in rgb)
    if not all(0 <= x <= 255 for x in (r, g, b)):
        raise ValueError(f"colour {rgb} outside 0..255")
    return (r << 16) | (g << 8) | b


def render_visbuf(mesh, w2c, H, W, fx, fy, cx, cy, segments=None, near=ZNEAR, far=ZFAR):
    """The visibility buffer int64 [K,H,W] (the kernels' uint64 words) of a DeviceMesh and device segments float32
    [S,2,3] at w2c float32 [K,3,4]: (fp32 depth bits << 32) | id, faces under their index, segment s under F + s,
    all ones (-1) where nothing is."""
    dev = mesh.vertices.device
    K, F = w2c.shape[0], mesh.faces.shape[0]
    vb = torch.empty(K, int(H), int(W), dtype=torch.int64, device=dev)
    L = _lib.lib()
    ws = torch.empty(L.gs_mesh_visbuf_workspace_bytes(), dtype=torch.uint8, device=dev)
    cam = (float(fx), float(fy), float(cx), float(cy), int(H), int(W), float(near), float(far))
    with torch.cuda.device(dev):
        st = _lib.stream_ptr(dev)
        _lib.check(L.gs_mesh_visbuf(_lib.ptr(mesh.vertices), mesh.vertices.shape[0], _lib.ptr(mesh.faces), F,
                                    _lib.ptr(w2c), K, *cam, _lib.ptr(vb), _lib.ptr(ws), ws.numel(), st), "mesh_visbuf")
        if segments is not None and segments.shape[0]:
            _lib.check(L.gs_line_visbuf(_lib.ptr(segments), segments.shape[0], F, _lib.ptr(w2c), K, *cam, _lib.ptr(vb),
                                        st), "line_visbuf")
    return vb


def resolve_visbuf(vb, mesh, w2c, fx, fy, cx, cy, line_colors=None, flat=False, ambient=0.3, diffuse=0.7,
                   background=(255, 255, 255), out=None):
    """The shaded image uint8 [K,H,W,3] of a visibility buffer (gs_visbuf_resolve)."""
    dev = vb.device
    K, H, W = vb.shape
    img = out if out is not None else torch.empty(K, H, W, 3, dtype=torch.uint8, device=dev)
    S = 0 if line_colors is None else line_colors.shape[0]
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().gs_visbuf_resolve(
            _lib.ptr(vb), K, H, W, _lib.ptr(mesh.vertices), mesh.vertices.shape[0], _lib.ptr(mesh.faces),
            mesh.faces.shape[0], _lib.ptr(w2c), float(fx), float(fy), float(cx), float(cy), _lib.ptr(mesh.colors),
            _lib.ptr(mesh.normals), int(bool(flat)), _lib.ptr(line_colors) if S else None, S, float(ambient),
            float(diffuse), _pack_rgb(background), _lib.ptr(img), _lib.stream_ptr(dev)), "visbuf_resolve")
    return img


def render_mesh_frames(mesh, c2w_list, H, W, fx, fy, cx, cy, lines=None, line_colors=None, near=ZNEAR, far=ZFAR,
                       flat=False, ambient=0.3, diffuse=0.7, background=(255, 255, 255), chunk=8, device=None):
    """Colour frames, a device uint8 [N,H,W,3], of `mesh` (None, a Mesh, (vertices, faces[, colours]) or an uploaded
    DeviceMesh) seen from c2w_list [N,4,4] (camera-to-world, OpenCV axes, inverted in float64), with the world-space
    segments `lines` [S,2,3] in `line_colors` [S,3] (uint8 levels, or floats in 0..1) drawn one pixel wide and depth-tested
    against the surface.  Shading: albedo * (ambient + diffuse * |cos(normal, pixel ray)|) with interpolated vertex
    normals, or the face's normal when `flat`; `background` where nothing is.  `chunk` poses per launch (a pose costs
    8 bytes per pixel of transient memory)."""
    dev = mesh.vertices.device if isinstance(mesh, DeviceMesh) else _device(device)
    mesh = upload_mesh(mesh, dev)
    c2w = _c2w_tensor(c2w_list)
    segs = cols = None
    if lines is not None and len(lines):
        segs = _as_tensor(lines, torch.float32, dev).reshape(-1, 2, 3)
        cols = line_colors
        if not isinstance(cols, torch.Tensor):
            cols = torch.from_numpy(np.ascontiguousarray(cols))
        if cols.dtype != torch.uint8:
            cols = torch.round(cols.double().clamp(0.0, 1.0) * 255.0)
        cols = cols.to(device=dev, dtype=torch.uint8).reshape(-1, 3).contiguous()
        if cols.shape[0] != segs.shape[0]:
            raise ValueError(f"render_mesh_frames: {cols.shape[0]} colours for {segs.shape[0]} segments")
    img = torch.empty(c2w.shape[0], int(H), int(W), 3, dtype=torch.uint8, device=dev)
    for s in range(0, c2w.shape[0], chunk):
        w2c = world_to_camera(c2w[s:s + chunk], dev)
        vb = render_visbuf(mesh, w2c, H, W, fx, fy, cx, cy, segs, near, far)
        resolve_visbuf(vb, mesh, w2c, fx, fy, cx, cy, cols, flat, ambient, diffuse, background, out=img[s:s + chunk])
    return img


class MeshVideo:
    """The reference's MeshVideo, synchronous and headless.  The viewer stands where the reference puts it (behind the
    first frame's pose, `viewer_extrinsic`) and never moves.  `height`, `width` (1080 x 1920, the reference's window) and
    `intrinsics` = (fx, fy, cx, cy) are ours to choose: the default is a 60 degree vertical field of view with the
    principal point at (W/2 - 0.5, H/2 - 0.5), our recollection of Open3D's default view, not verified against it.
    `near = 0` (the reference's default) means the rasteriser's near plane ZNEAR.  `frame()` is the last frame, a device
    uint8 [H,W,3]; `scene()` the line segments and colours it was drawn from.  `render=False` keeps the scene state only
    (no frame, no file, no GPU)."""

    def __init__(self, output, init_pose, cam_scale=1, save_rendering=False, near=0, estimate_c2w_list=None,
                 gt_c2w_list=None, height=1080, width=1920, intrinsics=None, device=None, render=True, **shading):
        self.output, self.cam_scale, self.save_rendering = output, cam_scale, save_rendering
        self.near = float(near) if near > 0 else ZNEAR
        self.estimate_c2w_list, self.gt_c2w_list = estimate_c2w_list, gt_c2w_list
        self.H, self.W = int(height), int(width)
        self.intrinsics = tuple(intrinsics) if intrinsics is not None else default_intrinsics(self.H, self.W)
        self.device, self.shading, self.render = device, shading, render
        if isinstance(init_pose, torch.Tensor):
            init_pose = init_pose.cpu().numpy()
        self.extrinsic = viewer_extrinsic(init_pose)
        self.view_c2w = np.linalg.inv(self.extrinsic)
        self.cameras = {}            # id -> [points [8,3], segments, colours, pose, the last transform applied]
        self.mesh = None
        self.traj_actor = self.traj_actor_gt = None
        self.frame_idx = 0
        self._frame = None

    # ---- the reference's surface -------------------------------------------------------
    def update_pose(self, index, pose, is_gt=False, is_keyframe=False):
        if isinstance(pose, torch.Tensor):
            pose = pose.cpu().numpy()
        pose[:3, 2] = -1             # the reference's, as it stands: the z column is overwritten, in place
        i = index + GT_ID_OFFSET if is_gt else index
        if i in self.cameras:
            actor = self.cameras[i]
            actor[4] = pose @ np.linalg.inv(actor[3])
            actor[0], actor[3] = transform_points(actor[0], actor[4]), pose
        else:
            pts, lines, cols = camera_actor(is_gt, is_keyframe, self.cam_scale)
            self.cameras[i] = [transform_points(pts, pose), lines, cols, pose, pose]
        self._tick()

    def update_mesh(self, path):
        self.mesh = load_mesh(path)
        if self.render:
            self.mesh = upload_mesh(self.mesh, self.device)
        self._tick()

    def update_cam_trajectory(self, c2w_list, is_gt):
        """`c2w_list` is, as in the reference, the index i up to which the trajectory is drawn."""
        actor = trajectory_actor(self.gt_c2w_list if is_gt else self.estimate_c2w_list, c2w_list, is_gt)
        if is_gt:
            self.traj_actor_gt = actor
        else:
            self.traj_actor = actor
        self._tick()

    def reset(self):
        self.cameras = {}
        self._tick()

    def start(self):
        if self.save_rendering:
            shutil.rmtree(os.path.join(self.output, "tmp_rendering"), ignore_errors=True)
        return self

    def join(self):
        if self._frame is not None:
            torch.cuda.synchronize(self._frame.device)

    # ---- ours ---------------------------------------------------------------------------
    def scene(self):
        """(segments float64 [S,2,3], colours float64 [S,3]) of every actor: the cameras in insertion order, then the
        estimated and the ground-truth trajectory."""
        actors = [(a[0], a[1], a[2]) for a in self.cameras.values()]
        actors += [a for a in (self.traj_actor, self.traj_actor_gt) if a is not None]
        segs = [pts[lines] for pts, lines, _ in actors if len(lines)]
        cols = [c for _, lines, c in actors if len(lines)]
        if not segs:
            return np.zeros((0, 2, 3)), np.zeros((0, 3))
        return np.concatenate(segs), np.concatenate(cols)

    def frame(self):
        return self._frame

    def _tick(self):
        if not self.render:
            return
        segs, cols = self.scene()
        fx, fy, cx, cy = self.intrinsics
        dev = self.mesh.vertices.device if self.mesh is not None else self.device
        self._frame = render_mesh_frames(self.mesh, self.view_c2w[None], self.H, self.W, fx, fy, cx, cy, lines=segs,
                                         line_colors=cols, near=self.near, device=dev, **self.shading)[0]
        if self.save_rendering:
            from PIL import Image
            self.frame_idx += 1
            os.makedirs(os.path.join(self.output, "tmp_rendering"), exist_ok=True)
            Image.fromarray(self._frame.cpu().numpy()).save(
                os.path.join(self.output, "tmp_rendering", f"{self.frame_idx:06d}.jpg"))
