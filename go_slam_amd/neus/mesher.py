"""Mesh culling on the GPU: the reference's `Mesher` (src/mesher.py) and `OrientedBoundingBox`
(src/oriented_bounding_box.py) without open3d, pyrender or trimesh.

- `render_mesh_depth`: `extract_depth_from_mesh` (src/mesher.py:444-480), batched depth rasterisation (gs_mesh_depth);
- `point_masks`: `Mesher.point_masks` (src/mesher.py:56-137), one launch per chunk of frames (gs_mesh_visibility);
- `face_components`: trimesh's `split(only_watertight=False)` labels plus fp64 component areas (gs_face_components,
  gs_face_component_areas);
- `OrientedBoundingBox`: Open3D's create_from_points (PCA of the convex-hull vertices) behind an exact device
  pre-filter (gs_hull_extremes, gs_hull_prefilter) so that qhull sees only the points that can be hull vertices.

Contracts: include/goslam_neus.h; tests/cull_restatement.py restates them on the CPU.  Deliberate differences from the
reference: exact fp32 depth with inclusive coverage instead of a 24-bit GL depth buffer; culled meshes keep
the input's face and vertex order (face masks) instead of being regrouped by component; no component above the area
threshold gives an empty Mesh.  align_mesh / eval_mesh at the end of a run: mesh_eval.py.
"""
import copy
import os

import numpy as np
import torch

from .. import _lib
from .mesh import Mesh, load_mesh
from .mesh_eval import align_mesh, eval_mesh

ZNEAR = 0.001
HULL_MARGIN = 1e-9          # relative margin of the interior test (qhull's plane rounding is far below it)


def _device(device=None):
    return torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())


def _as_tensor(x, dtype, device):
    if isinstance(x, torch.Tensor):
        return x.detach().to(device=device, dtype=dtype).contiguous()
    return torch.from_numpy(np.ascontiguousarray(x)).to(device=device, dtype=dtype).contiguous()


def _c2w_tensor(c2w_list):
    if isinstance(c2w_list, torch.Tensor):
        return c2w_list.detach().reshape(-1, 4, 4)
    if isinstance(c2w_list, np.ndarray):
        return torch.from_numpy(c2w_list).reshape(-1, 4, 4)
    return torch.stack([c.detach() if isinstance(c, torch.Tensor) else torch.as_tensor(c) for c in c2w_list])


def _mesh_arrays(mesh, device):
    if isinstance(mesh, Mesh):
        v, f = mesh.vertices, mesh.faces
    else:
        v, f = mesh
    return _as_tensor(v, torch.float32, device), _as_tensor(f, torch.int32, device)


def _render(verts, faces, c2w, H, W, fx, fy, cx, cy, far, out=None):
    """Depth maps [K,H,W] of one chunk of poses (c2w [K,4,4], any dtype/device)."""
    dev = verts.device
    w2c = torch.linalg.inv(c2w.to(device=dev, dtype=torch.float64))[:, :3, :].float().contiguous()
    K = w2c.shape[0]
    depth = out if out is not None else torch.empty(K, H, W, dtype=torch.float32, device=dev)
    L = _lib.lib()
    ws = torch.empty(L.gs_mesh_depth_workspace_bytes(), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(L.gs_mesh_depth(_lib.ptr(verts), verts.shape[0], _lib.ptr(faces), faces.shape[0], _lib.ptr(w2c), K,
                                   float(fx), float(fy), float(cx), float(cy), int(H), int(W), ZNEAR, float(far),
                                   _lib.ptr(depth), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)), "render_mesh_depth")
    return depth


def render_mesh_depth(mesh, c2w_list, H, W, fx, fy, cx, cy, far=20.0, chunk=256, device=None):
    """`extract_depth_from_mesh(mesh, c2w_list, H, W, fx, fy, cx, cy, far)` on the GPU: a device float32 [N,H,W], 0 where
    nothing is hit.  `mesh` is a Mesh or (vertices [V,3], faces [F,3]); c2w_list [N,4,4] camera-to-world (OpenCV), inverted
    in float64; `chunk` poses per launch."""
    dev = _device(device)
    verts, faces = _mesh_arrays(mesh, dev)
    c2w = _c2w_tensor(c2w_list)
    depth = torch.empty(c2w.shape[0], int(H), int(W), dtype=torch.float32, device=dev)
    for s in range(0, c2w.shape[0], chunk):
        _render(verts, faces, c2w[s:s + chunk], H, W, fx, fy, cx, cy, far, out=depth[s:s + chunk])
    return depth


def _visibility(points, depth, c2w, H, W, fx, fy, cx, cy, forecast_radius, seen, forecast):
    dev = points.device
    w2c = torch.inverse(c2w.to(device=dev, dtype=torch.float32)).contiguous()      # the reference's fp32 inverse
    depth = depth.to(device=dev, dtype=torch.float32).contiguous()
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().gs_mesh_visibility(_lib.ptr(points), points.shape[0], _lib.ptr(w2c), _lib.ptr(depth),
                                                 w2c.shape[0], float(fx), float(fy), float(cx), float(cy), int(H), int(W),
                                                 float(forecast_radius), _lib.ptr(seen), _lib.ptr(forecast),
                                                 _lib.stream_ptr(dev)), "point_masks")


def point_masks(vertices, depth, c2w_list, H, W, fx, fy, cx, cy, forecast_radius=0.0, chunk=256, device=None):
    """`Mesher.point_masks`: (seen, forecast) device bool [V] of vertices [V,3] against depth [N,H,W] at c2w_list [N,4,4];
    `chunk` frames per launch."""
    dev = _device(device)
    pts = _as_tensor(vertices, torch.float32, dev)
    c2w = _c2w_tensor(c2w_list)
    seen = torch.zeros(pts.shape[0], dtype=torch.uint8, device=dev)
    forecast = torch.zeros_like(seen)
    for s in range(0, c2w.shape[0], chunk):
        _visibility(pts, depth[s:s + chunk], c2w[s:s + chunk], H, W, fx, fy, cx, cy, forecast_radius, seen, forecast)
    return seen.bool(), forecast.bool()


def face_components(faces, vertices=None, device=None):
    """Edge-adjacency components of faces [F,3]: labels int32 [F] (the smallest face index of each component), and, when
    `vertices` [V,3] are given, also comp_area float64 [F] (indexed by label, 0 elsewhere) and the total area (float)."""
    dev = _device(device)
    f = _as_tensor(faces, torch.int32, dev).reshape(-1, 3)
    F = f.shape[0]
    L = _lib.lib()
    labels = torch.empty(F, dtype=torch.int32, device=dev)
    st = _lib.stream_ptr(dev)
    with torch.cuda.device(dev):
        ws = torch.empty(L.gs_face_components_workspace_bytes(F), dtype=torch.uint8, device=dev)
        _lib.check(L.gs_face_components(_lib.ptr(f), F, _lib.ptr(labels), _lib.ptr(ws), ws.numel(), st),
                   "face_components")
        del ws
        if vertices is None:
            return labels
        v = _as_tensor(vertices, torch.float64, dev).reshape(-1, 3)
        if F and (int(f.min()) < 0 or int(f.max()) >= v.shape[0]):
            raise ValueError(f"face_components: face indices outside [0, {v.shape[0]})")
        sorted_labels, perm = torch.sort(labels, stable=True)
        perm = perm.int()
        comp_area = torch.empty(F, dtype=torch.float64, device=dev)
        total = torch.zeros(1, dtype=torch.float64, device=dev)
        ws = torch.empty(max(16 * F, 1), dtype=torch.uint8, device=dev)
        _lib.check(L.gs_face_component_areas(_lib.ptr(v), _lib.ptr(f), F, _lib.ptr(perm), _lib.ptr(sorted_labels),
                                             _lib.ptr(comp_area), _lib.ptr(total), _lib.ptr(ws), ws.numel(), st),
                   "face_component_areas")
    return labels, comp_area, float(total.item())


def hull_candidates(points, device=None):
    """The exact pre-filter: the points (device float32 [n,3]) that can be vertices of their convex hull.  Extreme points
    along 13 directions (both signs) on the device, their hull by qhull (at most 26 points), then every point strictly
    inside all of its facets by more than the margin is discarded.  Returns (survivors [m,3] float32, the survivor
    mask)."""
    from scipy.spatial import ConvexHull
    from scipy.spatial import QhullError
    dev = _device(device) if not isinstance(points, torch.Tensor) or not points.is_cuda else points.device
    in64 = (points.dtype == torch.float64) if isinstance(points, torch.Tensor) else (np.asarray(points).dtype == np.float64)
    pts = _as_tensor(points, torch.float32, dev).reshape(-1, 3)
    n = pts.shape[0]
    keep = torch.ones(n, dtype=torch.uint8, device=dev)
    if n < 5:
        return pts, keep.bool()
    L = _lib.lib()
    st = _lib.stream_ptr(dev)
    idx = torch.empty(26, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        ws = torch.empty(L.gs_hull_extremes_workspace_bytes(n), dtype=torch.uint8, device=dev)
        _lib.check(L.gs_hull_extremes(_lib.ptr(pts), n, _lib.ptr(idx), _lib.ptr(ws), ws.numel(), st), "hull_extremes")
    ii = np.unique(idx.cpu().numpy())
    ii = ii[ii >= 0]
    ext = pts[torch.from_numpy(ii).to(dev).long()].double().cpu().numpy()
    try:
        hull = ConvexHull(ext)
    except (QhullError, ValueError):       # flat or too few extreme points: no interior to discard
        return pts, keep.bool()
    planes = np.ascontiguousarray(hull.equations, dtype=np.float64)          # n . p + c <= 0 inside, |n| = 1
    scale = float(np.abs(ext).max()) + float(np.abs(planes[:, 3]).max())
    # fp64 input was rounded to fp32 for the kernel: a coordinate moves by at most 2^-24 of itself
    margin = HULL_MARGIN * scale + (np.sqrt(3.0) * 2.0 ** -24 * scale if in64 else 0.0)
    pl = torch.from_numpy(planes).to(dev)
    with torch.cuda.device(dev):
        _lib.check(L.gs_hull_prefilter(_lib.ptr(pts), n, _lib.ptr(pl), planes.shape[0], margin, _lib.ptr(keep), st),
                   "hull_prefilter")
    mask = keep.bool()
    return pts[mask], mask


class OrientedBoundingBox(torch.nn.Module):
    """src/oriented_bounding_box.py with the same float64 buffers (center, R, extent) and state_dict."""

    def __init__(self):
        super().__init__()
        self.register_buffer('center', torch.zeros(3,).double())
        self.register_buffer('R', torch.zeros(3, 3).double())
        self.register_buffer('extent', torch.zeros(3,).double())
        self.survivors = None     # points the pre-filter passed to qhull in the last compute_from_pointcloud

    def compute_from_pointcloud(self, pointcloud, extend=0.0):
        """Open3D 0.13 OrientedBoundingBox.create_from_points + extend: the convex hull of the points (qhull, on the
        pre-filter's survivors), the population covariance of its vertices, R = its eigenvectors by decreasing
        eigenvalue, extent and centre from the hull vertices' box in that frame.  pointcloud: a device tensor or a NumPy
        array [n,3]."""
        from scipy.spatial import ConvexHull
        if isinstance(pointcloud, torch.Tensor) and pointcloud.is_cuda:
            full64 = pointcloud.dtype == torch.float64
        else:
            full64 = np.asarray(pointcloud).dtype == np.float64
        surv, mask = hull_candidates(pointcloud)
        self.survivors = int(surv.shape[0])
        if full64:       # qhull on the exact fp64 coordinates of the survivors
            src = pointcloud if isinstance(pointcloud, torch.Tensor) else torch.from_numpy(np.asarray(pointcloud))
            pts = src.reshape(-1, 3)[mask.to(src.device)].double().cpu().numpy()
        else:
            pts = surv.double().cpu().numpy()
        hull = ConvexHull(pts)
        hv = pts[hull.vertices]
        hv = hv[np.lexsort(hv.T[::-1])]      # a canonical order: the same vertex set always gives the same box
        mean = hv.mean(axis=0)
        d = hv - mean
        cov = d.T @ d / len(hv)
        evals, evecs = np.linalg.eigh(cov)
        R = np.ascontiguousarray(evecs[:, ::-1])
        q = d @ R
        lo, hi = q.min(axis=0), q.max(axis=0)
        center = R @ ((lo + hi) / 2.0) + mean
        dev = self.center.device
        self.center[:] = torch.from_numpy(center).to(dev)
        self.R[:] = torch.from_numpy(R).to(dev)
        self.extent[:] = torch.from_numpy(hi - lo).to(dev) + extend

    def in_bound(self, pointcloud):
        """Closed box test |R^T (p - center)|_i <= extent_i / 2 in float64 on the device.  Returns a NumPy bool array for
        NumPy input, a device bool tensor for a tensor."""
        dev = self.center.device if self.center.is_cuda else _device()
        p = _as_tensor(pointcloud, torch.float64, dev).reshape(-1, 3)
        d = p - self.center.to(dev)
        R = self.R.to(dev)
        local = d[:, 0:1] * R[0] + d[:, 1:2] * R[1] + d[:, 2:3] * R[2]     # elementwise: no fused or reordered sums
        inside = (local.abs() <= self.extent.to(dev) / 2.0).all(dim=1)
        return inside if isinstance(pointcloud, torch.Tensor) else inside.cpu().numpy()

    def get_axis_aligned_bounding_box(self):
        c = self.center.detach().cpu().numpy().astype(np.float64)
        R = self.R.detach().cpu().numpy().astype(np.float64)
        h = self.extent.detach().cpu().numpy().astype(np.float64) / 2.0
        signs = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], dtype=np.float64)
        corners = c[None, :] + (signs * h[None, :]) @ R.T
        return np.concatenate([corners.min(0).astype(np.float32)[:, None], corners.max(0).astype(np.float32)[:, None]],
                              axis=1)


class Mesher(object):
    """src/mesher.py `Mesher` with the same constructor, attributes and flow; meshing, culling, the bounding box and, at
    the end of a run with a ground-truth PLY, align_mesh / eval_mesh (mesh_eval.py) on the GPU."""

    def __init__(self, cfg, args, slam, points_batch_size=5e5):
        self.points_batch_size = int(points_batch_size)
        self.output = slam.output
        self.shared_mapping_net = slam.mapping_net
        self.video = slam.video
        self.reload_map = slam.reload_map
        self.scale = 1.0

        self.resolution = cfg['meshing']['resolution']
        self.level_set = cfg['meshing']['level_set']
        self.remove_small_geometry_threshold = cfg['meshing']['remove_small_geometry_threshold']
        self.get_largest_components = cfg['meshing']['get_largest_components']
        self.eval_rec = cfg['meshing']['eval_rec']
        self.n_points_to_eval = cfg['meshing']['n_points_to_eval']
        self.mesh_threshold_to_eval = cfg['meshing']['mesh_threshold_to_eval']
        self.gt_mesh_path = cfg['meshing']['gt_mesh_path']
        self.forecast_radius = cfg['meshing']['forecast_radius']

        assert self.forecast_radius >= 0, self.forecast_radius

        self.verbose = slam.verbose
        self.device = cfg['mapping']['device']
        self.pose_chunk = 256        # poses per depth / visibility launch: 79 MB of depth at 240 x 320

        os.makedirs(f'{self.output}/mesh/', exist_ok=True)

        self.H, self.W, self.fx, self.fy, self.cx, self.cy = slam.H, slam.W, slam.fx, slam.fy, slam.cx, slam.cy

    def _dev(self):
        d = torch.device(self.device)
        return d if d.index is not None else torch.device("cuda", torch.cuda.current_device())

    def point_masks(self, input_points, depth_list, estimate_c2w_list):
        """(seen, forecast) as NumPy bool arrays, like the reference."""
        if not isinstance(depth_list, torch.Tensor):
            depth_list = torch.stack([torch.as_tensor(d) for d in depth_list])
        seen, fc = point_masks(input_points, depth_list.to(self._dev()), estimate_c2w_list, self.H, self.W, self.fx,
                               self.fy, self.cx, self.cy, self.forecast_radius, self.pose_chunk, self._dev())
        return seen.cpu().numpy(), fc.cpu().numpy()

    def _cull_masks(self, mesh, estimate_c2w_list):
        """Depth maps and visibility chunk by chunk (no [N,H,W] stack is kept): (seen, forecast) device bool [V]."""
        dev = self._dev()
        verts, faces = _mesh_arrays(mesh, dev)
        c2w = _c2w_tensor(estimate_c2w_list)
        seen = torch.zeros(verts.shape[0], dtype=torch.uint8, device=dev)
        forecast = torch.zeros_like(seen)
        for s in range(0, c2w.shape[0], self.pose_chunk):
            part = c2w[s:s + self.pose_chunk]
            depth = _render(verts, faces, part, self.H, self.W, self.fx, self.fy, self.cx, self.cy, 20.0)
            _visibility(verts, depth, part, self.H, self.W, self.fx, self.fy, self.cx, self.cy, self.forecast_radius,
                        seen, forecast)
        return seen.bool(), forecast.bool()

    @torch.no_grad()
    def get_connected_mesh(self, mesh, get_largest_components=False):
        """Components by shared edges; the largest (ties to the lowest label), or every component whose area exceeds
        remove_small_geometry_threshold x the total.  The result keeps the input's face and vertex order; it is an empty
        Mesh when nothing passes."""
        out = mesh.copy()
        if len(mesh.faces) == 0:
            return out
        labels, comp_area, total = face_components(mesh.faces, mesh.vertices, self._dev())
        if get_largest_components:
            keep = labels == int(torch.argmax(comp_area))
        else:
            keep = (comp_area > self.remove_small_geometry_threshold * total)[labels.long()]
        out.update_faces(keep)
        out.remove_unreferenced_vertices()
        return out

    @torch.no_grad()
    def cull_mesh(self, mesh, estimate_c2w_list, bound, mesh_out_file):
        """src/mesher.py:155-240: bound cut (ndarray AABB +- 0.001, or an OrientedBoundingBox), projection culling,
        components, and the forecast mesh when forecast_radius > 0.  Writes bound_mesh.ply (with a bound),
        mesh_with_hole.ply, mesh_out_file and its _forecast twin; returns (cull_mesh, forecast_mesh).  `mesh` is cut in
        place by the bound, as in the reference."""
        if bound is not None:
            vertices = mesh.vertices[:, :3]
            if isinstance(bound, np.ndarray):
                eps = 0.001
                bound_mask = np.all(vertices >= (bound[:, 0] - eps), axis=1) & \
                    np.all(vertices <= (bound[:, 1] + eps), axis=1)
            else:
                bound_mask = bound.in_bound(np.asarray(vertices))
            mesh.update_faces(bound_mask[mesh.faces].all(axis=1))
            mesh.remove_unreferenced_vertices()
            mesh.export(f'{self.output}/mesh/bound_mesh.ply')

        seen, forecast = self._cull_masks(mesh, estimate_c2w_list)
        faces_d = torch.from_numpy(mesh.faces).to(seen.device)
        mesh_with_hole = mesh.copy()
        mesh_with_hole.update_faces(seen[faces_d].all(dim=1))
        mesh_with_hole.remove_unreferenced_vertices()
        mesh_with_hole.export(f'{self.output}/mesh/mesh_with_hole.ply')

        cull_mesh = self.get_connected_mesh(mesh_with_hole, self.get_largest_components)

        if abs(self.forecast_radius) > 0:
            forecast_mesh = mesh.copy()
            forecast_mesh.update_faces(forecast[faces_d].all(dim=1))
            forecast_mesh.remove_unreferenced_vertices()
            if len(cull_mesh.vertices):
                obb = OrientedBoundingBox().to(seen.device)
                obb.compute_from_pointcloud(cull_mesh.vertices)
                bound_mask = obb.in_bound(forecast_mesh.vertices)
            else:   # the reference has no mesh here; nothing bounds the forecast
                bound_mask = np.zeros(len(forecast_mesh.vertices), dtype=bool)
            forecast_mesh.update_faces(bound_mask[forecast_mesh.faces].all(axis=1))
            forecast_mesh.remove_unreferenced_vertices()
            forecast_mesh = self.get_connected_mesh(forecast_mesh, self.get_largest_components)
        else:
            forecast_mesh = cull_mesh.copy()

        cull_mesh.export(mesh_out_file)
        forecast_mesh.export(mesh_out_file.replace('.ply', '_forecast.ply'))
        return cull_mesh, forecast_mesh

    def update_param_from_mapping(self, the_end=False):
        """src/mesher.py:242-281: a copy of the mapping net, the keyframe count and c2w list, and at the end the OBB
        (extend 0.1) of the depth-filtered keyframe cloud -- iproj, depth_filter (count >= 3) and the far-point mask, all
        on the device."""
        from .. import droid_backends
        from ..lietorch_shim import SE3
        net = copy.deepcopy(self.shared_mapping_net).to(self.device)
        cur_idx = self.video.counter.value
        timestamp = self.video.timestamp[cur_idx - 1]
        aabb = None
        kf_c2w_list = SE3(self.video.poses.detach()[:cur_idx]).inv().matrix().data.cpu()

        if the_end:
            filter_thresh = 0.01
            filter_visible_num = 3
            dev = self.video.poses.device
            dirty_index = torch.arange(0, cur_idx).long().to(dev)
            poses = torch.index_select(self.video.poses.detach(), dim=0, index=dirty_index).contiguous()
            disps = torch.index_select(self.video.disps_up.detach(), dim=0, index=dirty_index).contiguous()
            intrinsic = (self.video.intrinsics[0].detach() * self.video.scale_factor).contiguous()
            w2w = SE3(self.video.pose_compensate[0].clone().unsqueeze(dim=0)).to(dev)

            points = droid_backends.iproj((w2w * SE3(poses).inv()).data.contiguous(), disps, intrinsic)
            thresh = filter_thresh * torch.ones_like(disps.mean(dim=[1, 2]))
            count = droid_backends.depth_filter(poses, disps, intrinsic, dirty_index, thresh)
            masks = (count >= filter_visible_num)
            masks = masks & (disps > 0.01 * disps.mean(dim=[1, 2], keepdim=True))
            sel_points = points.reshape(-1, 3)[masks.reshape(-1)]

            aabb = OrientedBoundingBox().to(dev)
            aabb.compute_from_pointcloud(sel_points, extend=0.1)

        return timestamp, cur_idx - 1, net, aabb, kf_c2w_list

    def __call__(self, the_end=False, estimate_c2w_list=None, gt_c2w_list=None, trans_init=None):
        if self.reload_map > 0 or the_end:
            timestamp, cur_idx, net, bound, kf_c2w_list = self.update_param_from_mapping(the_end=True)
            prefix = 'final_raw' if the_end else f'{int(timestamp):05d}'
            mesh_out_file = f'{self.output}/mesh/{prefix}_mesh.ply'

            mesh = net.extract_geometry(resolution=self.resolution, threshold=self.level_set, c2w_ref=None,
                                        save_path=None, color=True)
            mesh.export(mesh_out_file)

            if len(mesh.vertices) < 500:
                return

            c2w_list = estimate_c2w_list if estimate_c2w_list is not None else kf_c2w_list
            cull_mesh, forecast_mesh = self.cull_mesh(mesh=mesh, bound=bound, estimate_c2w_list=c2w_list,
                                                      mesh_out_file=mesh_out_file)

            if the_end and os.path.exists(self.gt_mesh_path) and self.gt_mesh_path.find('.ply') > -1:
                gt_mesh = load_mesh(self.gt_mesh_path)
                aligned_mesh, transformation = align_mesh(cull_mesh, gt_mesh, threshold=0.1, trans_init=trans_init,
                                                          return_transformation=True)
                aligned_mesh.export(f'{self.output}/mesh/aligned_mesh.ply')
                forecast_mesh.apply_transform(transformation)
                forecast_mesh.export(f'{self.output}/mesh/forecast_aligned_mesh.ply')
                if self.eval_rec:
                    eval_mesh(forecast_mesh, gt_mesh, N3d=self.n_points_to_eval, dist_th=self.mesh_threshold_to_eval,
                              out_path=f'{self.output}/metrics_mesh.txt')

            if self.verbose:
                print("\nINFO: Save mesh at {}!\n".format(mesh_out_file))

            del estimate_c2w_list, mesh, net, cull_mesh, forecast_mesh

            torch.cuda.empty_cache()

            self.reload_map -= 1
