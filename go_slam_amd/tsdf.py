"""Surfaces without the mapper: keyframe depth fused into a truncated signed distance volume and meshed on the GPU.

The reference has no such path -- under `only_tracking` it ends with a trajectory and a point cloud.  Here
csrc/tsdf.hip integrates depth maps at given world-to-camera poses into a dense lattice (one lane per lattice point, a
batch of frames per launch, no atomics), `neus.mesh.marching_cubes` meshes it, and a second kernel drops the vertices
next to never-observed points and colours the rest.  Arithmetic contract: include/goslam_hip.h (gs_tsdf_*);
tests/tsdf_restatement.py restates it serially.

csrc/tsdf_raycast.hip looks at the volume from a camera: `TSDFVolume.raycast` marches every pixel's ray to the first
zero crossing and returns depth, normal and colour images, and `eval_tsdf_depth` compares those depth images with the
sensor's at the end of a run (metrics_tsdf_depth.txt).  tests/tsdf_raycast_restatement.py restates the march (DESIGN.md
section 22).

csrc/esdf.hip answers what a robot asks of the map: `TSDFVolume.esdf` turns the volume into an `ESDF`, the exact
Euclidean distance to the nearest surface lattice point at every lattice point, `ESDF.query` interpolates it and its
gradient at world points, `ESDF.occupancy_slice` / `save_map` flatten a slab into a map_server occupancy map, and
`trajectory_clearance` reports how close the estimated camera centres come to the fused surfaces
(metrics_tsdf_clearance.txt).  tests/esdf_restatement.py restates the field.

csrc/geodesic.hip answers where to go: `ESDF.passable` marks the lattice points a robot of a given radius may occupy,
`ESDF.plan` finds the shortest collision-free route between two world points and `ESDF.reachable` what can be reached
at all (plan.py: the cost-to-go field and the walk down it; tests/geodesic_restatement.py).

csrc/frontier.hip answers what has not been seen: `ESDF.frontiers` groups the free lattice points that border
never-observed space into clusters, each priced by the route to it, and `ESDF.explore` picks one and plans the way there
(frontier.py: marking, labelling and the cluster table; tests/frontier_restatement.py).

csrc/tsdf_align.hip answers where a camera is: `TSDFVolume.align` moves given poses until a depth image's pixels lie on
the volume's surface, `pose_scores` measures the fit, `localize.relocalize` finds a pose among candidates, `save` / `load`
carry a volume to another run, and metrics_tsdf_align.txt reports how far a run's poses disagree with the surface they
produced (localize.py; tests/tsdf_align_restatement.py).

csrc/tsdf_merge.hip puts two volumes together: `TSDFVolume.register` finds the transform that lays another volume's
surfaces onto this one's, `TSDFVolume.merge` fuses another volume into this one, `tsdf_merge.join_volumes` makes one map
of several sessions' volumes, and cfg["tsdf"]["merge"] joins a run's volume with an earlier run's saved one
(tsdf_merge.py; tests/tsdf_merge_restatement.py).

csrc/tsdf_planes.hip finds what is level: `TSDFVolume.find_planes` returns the volume's dominant planes,
`tsdf_planes.floor_plane` picks the floor, `TSDFVolume.upright` resamples the volume into a frame that stands on it, and
cfg["tsdf"]["planes"] / cfg["tsdf"]["upright"] report the planes of a run and hand the navigation keys the upright volume
(tsdf_planes.py; tests/tsdf_planes_restatement.py).

csrc/tsdf_objects.hip finds what is everything else: `TSDFVolume.find_objects` returns the clusters of surface samples that
lie on none of the structure planes, each with an oriented box, and cfg["tsdf"]["objects"] writes a run's map/objects.txt
(tsdf_objects.py; tests/tsdf_objects_restatement.py).

csrc/rooms.hip answers which rooms there are: `ESDF.rooms` splits the space a robot may occupy by clearance into rooms,
finds the doorways between them and the graph of both, and cfg["tsdf"]["esdf"]["rooms"] writes a run's map/rooms.txt
(rooms.py; tests/rooms_restatement.py).

tsdf_live.py keeps such a volume during a run, while the poses still move; it fuses through
`keyframe_observations`, the rule `fuse_keyframes` applies per chunk.  tsdf_run.py is the end-of-run step that serves the
cfg["tsdf"] keys above, one stage per key (`fuse_from_config`).
"""
import math
import os

import numpy as np
import torch

from . import _lib
from . import floor as _floor
from . import follow as _follow
from . import frontier as _frontier
from . import localize as _localize
from . import plan as _plan
from . import rooms as _rooms
from . import tsdf_merge as _merge
from . import tsdf_objects as _objects
from . import tsdf_planes as _planes
from . import view as _view
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


def c2w_matrices(w2c):
    """float32 [K,3,4] camera-to-world matrices from world-to-camera poses in the forms `w2c_matrices` accepts ([K,7],
    [K,4,4], [K,3,4]; rigid).  The inverse (R^T, -R^T t) is formed in float64 on the tensor's device and rounded once."""
    w2c = torch.as_tensor(w2c)
    if w2c.dim() == 2 and w2c.shape[1] == 7:
        m = SE3(w2c.double()).inv().matrix()[:, :3, :]
    elif w2c.dim() == 3 and tuple(w2c.shape[1:]) in ((4, 4), (3, 4)):
        rt = w2c[:, :3, :3].double().transpose(1, 2)
        m = torch.cat([rt, -(rt @ w2c[:, :3, 3:].double())], dim=2)
    else:
        raise ValueError(f"w2c must be [K,7], [K,4,4] or [K,3,4] (got {tuple(w2c.shape)})")
    return m.to(torch.float32).contiguous()


def _intrinsics4(intrinsics, what):
    intr = list(intrinsics) if isinstance(intrinsics, (tuple, list)) else \
        torch.as_tensor(intrinsics).detach().cpu().reshape(-1).tolist()
    if len(intr) != 4:
        raise ValueError(f"{what}: intrinsics must be (fx, fy, cx, cy)")
    return [float(v) for v in intr]


def fusion_inputs(what, dev, depth, w2c, intrinsics, images=None, mask=None):
    """The frames `TSDFVolume.integrate` and `ReversibleTSDF.accumulate` take, checked on the host -- depth [K,H,W], K
    poses, images [K,3,H,W], mask [K,H,W], four intrinsics; ValueError under the caller's name `what` -- and only then
    moved to `dev` as contiguous float32 -> (K, H, W, depth, [K,3,4] matrices, images, mask, [fx, fy, cx, cy])."""
    depth = torch.as_tensor(depth)
    if depth.dim() != 3:
        raise ValueError(f"{what}: depth must be [K,H,W] (got {list(depth.shape)})")
    K, H, W = (int(s) for s in depth.shape)
    w2c = torch.as_tensor(w2c)
    if w2c.dim() > 0 and w2c.shape[0] != K:
        raise ValueError(f"{what}: {w2c.shape[0]} poses for {K} depth maps")
    frames = [depth]
    for t, name, shape in ((images, "images", (K, 3, H, W)), (mask, "mask", (K, H, W))):
        t = None if t is None else torch.as_tensor(t)
        if t is not None and tuple(t.shape) != shape:
            raise ValueError(f"{what}: {name} must be {list(shape)} (got {list(t.shape)})")
        frames.append(t)
    intr = _intrinsics4(intrinsics, what)
    mats = w2c_matrices(w2c).to(dev)
    depth, images, mask = (None if t is None else t.to(device=dev, dtype=torch.float32).contiguous() for t in frames)
    return K, H, W, depth, mats, images, mask, intr


def lattice(bound, voxel_size, trunc, what):
    """(voxel, lo float64 [3], dims, trunc) of the lattice over `bound` ([3,2]: lo, hi per axis): points at
    lo + idx * voxel, n = ceil((hi - lo) / voxel) + 1 per axis, truncation 4 voxels unless given.  ValueError for a bad
    bound or voxel, an empty axis or one with more than MAX_POINTS points."""
    bound = np.asarray(bound.detach().cpu() if isinstance(bound, torch.Tensor) else bound, dtype=np.float64)
    if bound.shape != (3, 2):
        raise ValueError(f"{what}: bound must be [3,2] (got {bound.shape})")
    voxel = float(voxel_size)
    if not voxel > 0:
        raise ValueError(f"{what}: voxel_size must be positive (got {voxel_size})")
    dims = []
    for axis, name in enumerate("xyz"):
        n = int(math.ceil((bound[axis, 1] - bound[axis, 0]) / voxel)) + 1
        if n > MAX_POINTS:
            raise ValueError(f"{what}: axis {name} needs {n} lattice points at voxel_size {voxel} "
                             f"(at most {MAX_POINTS}); enlarge voxel_size or shrink the bound")
        if n < 2:
            raise ValueError(f"{what}: axis {name} of the bound is empty")
        dims.append(n)
    return voxel, bound[:, 0].copy(), tuple(dims), 4.0 * voxel if trunc is None else float(trunc)


class TSDFVolume:
    """A dense TSDF over `bound` ([3,2]: lo, hi per axis) with lattice points at lo + idx * voxel_size,
    n = ceil((hi - lo) / voxel_size) + 1 per axis.  `.tsdf` (+1 where nothing was seen) and `.weight` are float32
    [nx,ny,nz], `.colors` float32 [3,nx,ny,nz], on `device`."""

    def __init__(self, bound, voxel_size, trunc=None, max_weight=64.0, device=None):
        self.voxel, self.lo, self.dims, self.trunc = lattice(bound, voxel_size, trunc, "TSDFVolume")
        self.max_weight = float(max_weight)
        if not self.trunc > 0 or not self.max_weight >= 1:
            raise ValueError(f"TSDFVolume: trunc {self.trunc} must be positive and max_weight {self.max_weight} >= 1")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.tsdf = torch.empty(self.dims, dtype=torch.float32, device=self.device)
        self.weight = torch.empty(self.dims, dtype=torch.float32, device=self.device)
        self.colors = torch.empty((3,) + self.dims, dtype=torch.float32, device=self.device)
        self._flags = None         # raycast's brick flags, dropped by whatever changes tsdf (reset, integrate)
        self.reset()

    def reset(self):
        self._flags = None
        self.tsdf.fill_(1.0)
        self.weight.zero_()
        self.colors.zero_()

    @torch.no_grad()
    def integrate(self, depth, w2c, intrinsics, images=None, mask=None):
        """Fuse K frames in order: depth [K,H,W] in metres (<= 0 invalid), w2c [K,7] / [K,4,4] / [K,3,4],
        intrinsics (fx, fy, cx, cy) of the depth maps, images [K,3,H,W] in [0,1] and mask [K,H,W] (0 drops a pixel)
        optional.  Enqueues ceil(K / batch) launches on the current stream; nothing is read back."""
        dev = self.device
        K, H, W, depth, mats, images, mask, intr = fusion_inputs("TSDFVolume.integrate", dev, depth, w2c, intrinsics,
                                                                 images, mask)
        if K == 0:
            return self
        nx, ny, nz = self.dims
        self._flags = None
        with torch.cuda.device(dev):
            rc = _lib.lib().gs_tsdf_integrate(
                _lib.ptr(self.tsdf), _lib.ptr(self.weight), _lib.ptr(self.colors), nx, ny, nz, _lib.ptr(depth),
                _lib.ptr(mask), _lib.ptr(images), _lib.ptr(mats), K, H, W, *intr,
                float(self.lo[0]), float(self.lo[1]), float(self.lo[2]), self.voxel, self.trunc, self.max_weight,
                _lib.stream_ptr(dev))
        _lib.check(rc, "TSDFVolume.integrate")
        return self

    @torch.no_grad()
    def brick_flags(self):
        """uint8 [bx,by,bz], b = ceil((n - 1) / 8): 1 where a brick of 8 x 8 x 8 cells has a corner with tsdf < 0
        (gs_tsdf_brick_flags).  Kept until `integrate` or `reset` changes the volume; code that writes `.tsdf` itself
        sets `_flags = None` afterwards."""
        if self._flags is None:
            nx, ny, nz = self.dims
            flags = torch.empty(tuple((n - 1 + 7) // 8 for n in self.dims), dtype=torch.uint8, device=self.device)
            assert flags.numel() == _lib.lib().gs_tsdf_brick_flags_bytes(nx, ny, nz)
            with torch.cuda.device(self.device):
                rc = _lib.lib().gs_tsdf_brick_flags(_lib.ptr(self.tsdf), nx, ny, nz, _lib.ptr(flags),
                                                    _lib.stream_ptr(self.device))
            _lib.check(rc, "TSDFVolume.brick_flags")
            self._flags = flags
        return self._flags

    @torch.no_grad()
    def raycast(self, w2c, intrinsics, size, near=0.0, far=math.inf, step=0.5, min_weight=1.0, color=True, skip=True):
        """The first zero crossing of the volume along every pixel's ray (gs_tsdf_raycast): {"depth": [K,H,W] in metres
        along the optical axis, 0 without a hit, "normal": [K,H,W,3] unit, world frame, toward free space, "color":
        [K,H,W,3] or None}, float32 on the volume's device.  w2c as `integrate` takes it (one pose list serves both);
        intrinsics (fx, fy, cx, cy) of the size = (H, W) images; `step` is the march's step in voxels, in (0, 1]; a cell
        counts only where all eight corners were seen `min_weight` times.  skip=False marches without the brick flags:
        same bits, slower.  Enqueues on the current stream; nothing is read back.  ValueError for bad shapes or ranges."""
        return self._raycast(c2w_matrices(w2c), intrinsics, size, near, far, step, min_weight, color, skip)

    def _raycast(self, c2w, intrinsics, size, near=0.0, far=math.inf, step=0.5, min_weight=1.0, color=True, skip=True):
        """`raycast` from float32 [K,3,4] camera-to-world matrices."""
        what = "TSDFVolume.raycast"
        intr = _intrinsics4(intrinsics, what)
        if len(tuple(size)) != 2 or int(size[0]) < 1 or int(size[1]) < 1:
            raise ValueError(f"{what}: size must be (H, W) with H, W >= 1 (got {size})")
        H, W = int(size[0]), int(size[1])
        near, far, step, min_weight = float(near), float(far), float(step), float(min_weight)
        if not (intr[0] != 0 and intr[1] != 0):
            raise ValueError(f"{what}: fx and fy must not be zero")
        if not (near >= 0 and far > near):
            raise ValueError(f"{what}: need 0 <= near < far (got near {near}, far {far})")
        if not (0 < step <= 1):
            raise ValueError(f"{what}: step must lie in (0, 1] voxels (got {step})")
        if math.ceil(sum(self.dims) / step) + 2 > 2 ** 24:
            raise ValueError(f"{what}: step {step} needs more than 2^24 steps across this lattice")
        if c2w.dim() != 3 or tuple(c2w.shape[1:]) != (3, 4):
            raise ValueError(f"{what}: camera-to-world matrices must be [K,3,4] (got {list(c2w.shape)})")
        dev = self.device
        c2w = c2w.to(device=dev, dtype=torch.float32).contiguous()
        K = int(c2w.shape[0])
        depth = torch.empty(K, H, W, dtype=torch.float32, device=dev)
        normal = torch.empty(K, H, W, 3, dtype=torch.float32, device=dev)
        rgb = torch.empty(K, H, W, 3, dtype=torch.float32, device=dev) if color else None
        if K > 0:
            flags = self.brick_flags() if skip else None
            nx, ny, nz = self.dims
            with torch.cuda.device(dev):
                rc = _lib.lib().gs_tsdf_raycast(
                    _lib.ptr(self.tsdf), _lib.ptr(self.weight), _lib.ptr(self.colors) if color else None, nx, ny, nz,
                    _lib.ptr(flags), _lib.ptr(c2w), K, H, W, *intr, float(self.lo[0]), float(self.lo[1]),
                    float(self.lo[2]), self.voxel, near, far, step, min_weight, _lib.ptr(depth), _lib.ptr(normal),
                    _lib.ptr(rgb), _lib.stream_ptr(dev))
            _lib.check(rc, what)
        return {"depth": depth, "normal": normal, "color": rgb}

    def align(self, depth, c2w_init, intrinsics, frame=None, levels=_localize.DEFAULT_LEVELS, huber=0.5,
              max_depth=math.inf, min_weight=1.0, lam_rel=1e-6, lam_abs=1e-9, min_count=64):
        """Where were these depth images taken from?  B camera-to-world poses refined by direct alignment to this volume
        (gs_tsdf_align_system / gs_tsdf_align_step), coarse to fine over `levels` = (pixel stride, iterations) pairs: see
        `localize.align` for the arguments and the returned dict (c2w, ok, rmse_m, inlier_fraction, count, trace, moved_m,
        moved_deg; host arrays, one read)."""
        return _localize.align(self, depth, c2w_init, intrinsics, frame, levels, huber, max_depth, min_weight, lam_rel,
                               lam_abs, min_count)

    def pose_scores(self, depth, c2w, intrinsics, frame=None, stride=4, huber=0.5, max_depth=math.inf, min_weight=1.0):
        """How well do these poses explain the depth images?  One gs_tsdf_align_system per pose and no step ->
        {"rmse_m", "inlier_fraction", "count"} (`localize.pose_scores`)."""
        return _localize.pose_scores(self, depth, c2w, intrinsics, frame, stride, huber, max_depth, min_weight)

    def register(self, other, T_init, levels=_merge.DEFAULT_LEVELS, huber=0.5, min_weight=1.0, lam_rel=1e-6, lam_abs=1e-9,
                 min_count=64):
        """Where does the volume `other` sit in this one?  B transforms other's world to this volume's world refined by
        direct alignment of the two lattices (gs_tsdf_register_system / gs_tsdf_align_step), coarse to fine over `levels`
        = (lattice stride, iterations) pairs: see `tsdf_merge.register_volumes` for the arguments and the returned dict
        (T, ok, rmse_m, overlap, count, trace, moved_m, moved_deg, moved_constrained_m, n_constrained; host arrays, one
        read)."""
        return _merge.register_volumes(self, other, T_init, levels, huber, min_weight, lam_rel, lam_abs, min_count)

    def merge(self, other, T=None, min_weight=1.0):
        """Fuse the volume `other` into this one in place (gs_tsdf_merge) at the transform T, other's world to this
        volume's ([3,4] / [4,4]; None: the identity): see `tsdf_merge.merge_volume`.  Drops the brick flags and returns
        self."""
        return _merge.merge_volume(self, other, T, min_weight)

    def find_planes(self, bins=16, cone_deg=10.0, band=None, max_planes=8, min_cells=64, min_weight=1.0, iterations=3):
        """The dominant planes of the volume (gs_tsdf_plane_votes / _offsets / _moments), by descending inlier count: a
        list of {"normal" (unit, toward free space), "offset", "count", "rmse_m", "centroid", "area_m2"}: see
        `tsdf_planes.find_planes`.  `tsdf_planes.floor_plane` picks the floor among them."""
        return _planes.find_planes(self, bins, cone_deg, band, max_planes, min_cells, min_weight, iterations)

    def upright(self, plane=None, up_hint=None, up_axis=2, up_sign=+1, heading=None, voxel_size=None, **find_args):
        """(a new TSDFVolume, T float64 [4,4] world to map): this volume resampled into a frame whose `up_axis` is the
        normal of `plane` and whose coordinate 0 along it is the plane; plane=None finds the floor under `up_hint`
        (`find_planes(**find_args)`, `floor_plane`); heading="walls" also lays the largest wall along a lattice axis: see
        `tsdf_planes.upright_volume`.  The navigation calls (`esdf`, `occupancy_slice`, `plan`, `frontiers`,
        `next_view`) then take up_axis and heights above the floor."""
        return _planes.upright_volume(self, plane, up_hint, up_axis, up_sign, heading, voxel_size, **find_args)

    def find_objects(self, planes, up=None, cone_deg=10.0, band=None, min_cells=16, min_weight=1.0, max_sweeps=65536):
        """What stands on none of the structure planes `planes` (`tsdf_objects.structure_planes` of `find_planes`' planes):
        an `Objects` with the object cells' clusters, their table and `.boxes`, one oriented box per cluster of at least
        min_cells cells (gs_tsdf_object_mark / _table / _extents, gs_frontier_relax): see `tsdf_objects.find_objects`."""
        return _objects.find_objects(self, planes, up, cone_deg, band, min_cells, min_weight, max_sweeps)

    def save(self, path):
        """Write the volume as one .npz (tsdf, weight, colors, lo, voxel, trunc, max_weight, dims); `load` gives the same
        bits back."""
        _localize.save_volume(self, path)

    @classmethod
    def load(cls, path, device=None):
        """The volume `save` wrote, on `device`; ValueError for a file whose arrays disagree with its dims."""
        return _localize.load_volume(cls, path, device)

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

    @torch.no_grad()
    def esdf(self, max_distance=None, min_weight=1.0):
        """The Euclidean distance field of the volume as it is now (gs_esdf_build): an `ESDF` snapshot.  Distances are
        exact up to `max_distance` metres, R = ceil(max_distance / voxel) voxels in [1, 1023], and capped there; None
        means R = 1023, which is exact and unbounded on any permitted lattice.  A point counts as seen with weight >=
        `min_weight`.  Enqueues on the current stream, reads nothing back and leaves the volume untouched.  ValueError
        for a bad max_distance or min_weight, before the device is touched."""
        what = "TSDFVolume.esdf"
        if max_distance is None:
            radius = ESDF_MAX_RADIUS
        else:
            max_distance = float(max_distance)
            if not (max_distance > 0 and math.isfinite(max_distance)):
                raise ValueError(f"{what}: max_distance must be positive and finite (got {max_distance})")
            radius = int(math.ceil(max_distance / self.voxel))
            if not 1 <= radius <= ESDF_MAX_RADIUS:
                raise ValueError(f"{what}: max_distance {max_distance} is {radius} voxels of {self.voxel} m "
                                 f"(at most {ESDF_MAX_RADIUS}); pass None for an unbounded field")
        min_weight = float(min_weight)
        if math.isnan(min_weight):
            raise ValueError(f"{what}: min_weight is NaN")
        dev = self.device
        state = torch.empty(self.dims, dtype=torch.uint8, device=dev)
        d2 = torch.empty(self.dims, dtype=torch.int32, device=dev)
        dist = torch.empty(self.dims, dtype=torch.float32, device=dev)
        nx, ny, nz = self.dims
        with torch.cuda.device(dev):
            rc = _lib.lib().gs_esdf_build(_lib.ptr(self.tsdf), _lib.ptr(self.weight), nx, ny, nz, min_weight, radius,
                                          self.voxel, _lib.ptr(state), _lib.ptr(d2), _lib.ptr(dist), _lib.stream_ptr(dev))
        _lib.check(rc, what)
        return ESDF(state, d2, dist, self.lo, self.voxel, self.dims, radius)


ESDF_MAX_RADIUS = MAX_POINTS - 1     # voxels: no two points of a permitted lattice are further apart along an axis
MAP_FREE, MAP_OCCUPIED, MAP_UNKNOWN = 254, 0, 205      # the trinary values of a ROS map_server PGM


class ESDF:
    """A snapshot of a TSDFVolume's distance field (TSDFVolume.esdf); it does not refer back to the volume.  On the
    volume's lattice (`lo`, `voxel`, `dims`): `.state` uint8 (0 unknown, 1 free, 2 solid), `.d2` int32, the squared
    distance in voxels to the nearest site (a lattice point next to a sign change; 0x7fffffff beyond `radius_voxels`),
    `.dist` float32 in metres, negative inside solid, +-radius_voxels * voxel beyond the band."""

    def __init__(self, state, d2, dist, lo, voxel, dims, radius_voxels):
        self.state, self.d2, self.dist = state, d2, dist
        self.lo = np.array(lo, dtype=np.float64)
        self.voxel = float(voxel)
        self.dims = tuple(int(n) for n in dims)
        self.radius_voxels = int(radius_voxels)
        self.device = dist.device

    @torch.no_grad()
    def query(self, points):
        """The field at world points [N,3] (gs_esdf_query): {"dist": float32 [N], the trilinear interpolant, "grad":
        float32 [N,3], its analytic gradient (not normalised; toward free space), "valid": bool [N], the point lies in
        a cell of the lattice, "known": bool [N], all eight corners of that cell were seen}.  Invalid points hold
        zeros.  Enqueues on the current stream; nothing is read back."""
        points = torch.as_tensor(points)
        if points.dim() != 2 or points.shape[1] != 3:
            raise ValueError(f"ESDF.query: points must be [N,3] (got {list(points.shape)})")
        dev = self.device
        points = points.to(device=dev, dtype=torch.float32).contiguous()
        N = int(points.shape[0])
        dist = torch.empty(N, dtype=torch.float32, device=dev)
        grad = torch.empty(N, 3, dtype=torch.float32, device=dev)
        flags = torch.empty(N, dtype=torch.uint8, device=dev)
        if N > 0:
            nx, ny, nz = self.dims
            with torch.cuda.device(dev):
                rc = _lib.lib().gs_esdf_query(_lib.ptr(self.dist), _lib.ptr(self.state), nx, ny, nz, float(self.lo[0]),
                                              float(self.lo[1]), float(self.lo[2]), self.voxel, _lib.ptr(points), N,
                                              _lib.ptr(dist), _lib.ptr(grad), _lib.ptr(flags), _lib.stream_ptr(dev))
            _lib.check(rc, "ESDF.query")
        return {"dist": dist, "grad": grad, "valid": (flags & 1) != 0, "known": (flags & 2) != 0}

    def slice_arguments(self, up_axis, height, robot_radius=0.0, known_fraction=0.5):
        """(up_axis, k0, k1, occ_d2, min_known) of gs_esdf_slice for `occupancy_slice`'s arguments, or ValueError."""
        what = "ESDF.occupancy_slice"
        if isinstance(up_axis, bool) or not isinstance(up_axis, (int, np.integer)) or not 0 <= int(up_axis) <= 2:
            raise ValueError(f"{what}: up_axis must be 0, 1 or 2 (got {up_axis!r})")
        a = int(up_axis)
        try:
            h0, h1 = (float(h) for h in height)
        except (TypeError, ValueError):
            raise ValueError(f"{what}: height must be (h0, h1) in metres (got {height!r})") from None
        robot_radius, known_fraction = float(robot_radius), float(known_fraction)
        if math.isnan(h0) or math.isnan(h1):
            raise ValueError(f"{what}: height {height!r} holds NaN")
        top = self.dims[a] - 1
        k0 = 0 if h0 == -math.inf else int(max(math.ceil(min((h0 - self.lo[a]) / self.voxel, top + 1.0)), 0))
        k1 = top if h1 == math.inf else int(min(math.floor(max((h1 - self.lo[a]) / self.voxel, -1.0)), top))
        if k0 > k1:
            raise ValueError(f"{what}: no lattice layer of axis {a} lies in [{h0}, {h1}] m (the axis spans "
                             f"[{self.lo[a]}, {self.lo[a] + top * self.voxel}] in steps of {self.voxel})")
        if not 0 <= robot_radius <= self.radius_voxels * self.voxel:
            raise ValueError(f"{what}: robot_radius {robot_radius} m outside [0, {self.radius_voxels * self.voxel}], "
                             "the band of this field (build it with a larger max_distance)")
        if not 0 <= known_fraction <= 1:
            raise ValueError(f"{what}: known_fraction must lie in [0, 1] (got {known_fraction})")
        occ_d2 = int(math.floor((robot_radius / self.voxel) ** 2))
        min_known = int(math.ceil(known_fraction * (k1 - k0 + 1)))
        return a, k0, k1, occ_d2, min_known

    @torch.no_grad()
    def occupancy_slice(self, up_axis, height, robot_radius=0.0, known_fraction=0.5):
        """The 2-D map of the slab of lattice layers k along `up_axis` with height[0] <= lo + k * voxel <= height[1]
        (gs_esdf_slice).  The two other axes, in increasing order, index the images [n_u, n_v].  A column is occupied
        (cells 0) when a point of it is solid or within `robot_radius` of a site, else free (254) when at least
        `known_fraction` of its points were seen, else unknown (205).  -> {"cells": uint8 [n_u,n_v], "clearance":
        float32 [n_u,n_v], the smallest dist of the column in metres, "origin": (x, y), the corner of cell (0, 0) along
        the two image axes (its lattice point minus half a voxel: map_server's origin), "resolution": the voxel, "axes":
        (u, v)}, images on the field's device.  ValueError for an empty range or a radius beyond the field's band."""
        a, k0, k1, occ_d2, min_known = self.slice_arguments(up_axis, height, robot_radius, known_fraction)
        u, v = [ax for ax in range(3) if ax != a]
        dev = self.device
        cells = torch.empty((self.dims[u], self.dims[v]), dtype=torch.uint8, device=dev)
        clearance = torch.empty((self.dims[u], self.dims[v]), dtype=torch.float32, device=dev)
        nx, ny, nz = self.dims
        with torch.cuda.device(dev):
            rc = _lib.lib().gs_esdf_slice(_lib.ptr(self.state), _lib.ptr(self.d2), _lib.ptr(self.dist), nx, ny, nz, a, k0,
                                          k1, occ_d2, min_known, _lib.ptr(cells), _lib.ptr(clearance),
                                          _lib.stream_ptr(dev))
        _lib.check(rc, "ESDF.occupancy_slice")
        return {"cells": cells, "clearance": clearance, "resolution": self.voxel, "axes": (u, v),
                "origin": (float(self.lo[u] - 0.5 * self.voxel), float(self.lo[v] - 0.5 * self.voxel))}

    def floor_arguments(self, up_axis, height, robot_radius, robot_height, step_height, up_sign=+1):
        """(up_axis, up_sign, p0, p1, H, S, R2) of gs_floor_columns and gs_floor_footprint for `floor_map`'s arguments, or
        ValueError.  Touches no device."""
        what = "ESDF.floor_map"
        a, sign = _floor._axis_sign(up_axis, up_sign, what)
        _, k0, k1, _, _ = self.slice_arguments(a, height)
        H, S, R2 = _floor.robot_arguments(self.voxel, robot_radius, robot_height, step_height, what)
        top = self.dims[a] - 1
        p0, p1 = (k0, k1) if sign > 0 else (top - k1, top - k0)
        return a, sign, p0, p1, H, S, R2

    @torch.no_grad()
    def floor_map(self, up_axis, height, robot_radius, robot_height, step_height, up_sign=+1):
        """The map of where a ground robot can stand and roll (floor.columns, floor.footprint): a
        disc of `robot_radius` metres, `robot_height` metres tall, that takes steps of `step_height` metres, on the floor
        whose stand cells lie in the layers with height[0] <= lo + k * voxel <= height[1] along `up_axis` (`up_sign` -1:
        up is the axis' negative direction).  A column is drivable (cells 254) when under the whole disc there is seen
        support with free headroom and no height difference above the step; occupied (0) when the disc meets a column
        without floor -- a wall, a table too low, a hole seen free to the bottom -- or a step too high; else unknown
        (205): floor or headroom not observed yet.  -> `occupancy_slice`'s dict {"cells", "origin", "resolution", "axes"}
        with "floor" int16 [n_u,n_v] (the lattice index of the stand cell, -1 without), "floor_height" float32 (the world
        coordinate along up of its lower face, NaN without), "kind" uint8 (0 never observed, 1 floor, 2 maybe, 3 none),
        "why" uint8 (of an occupied column: 1 no floor, 2 no floor under the disc, 3 a step), "rough" int16 (the largest
        height difference under the disc in cells), "up_axis" and "up_sign"; images on the field's device.  H =
        ceil(robot_height / voxel), S = floor(step_height / voxel), R2 = floor((robot_radius / voxel)^2).  Enqueues on
        the current stream and reads nothing back.  ValueError for an empty range, a value that is not finite or
        negative, or a radius below sqrt(2) or above 32 cells, before the device is touched."""
        a, sign, p0, p1, H, S, R2 = self.floor_arguments(up_axis, height, robot_radius, robot_height, step_height, up_sign)
        u, v = [ax for ax in range(3) if ax != a]
        floor, kind = _floor.columns(self.state, a, sign, p0, p1, H)
        cells, why, rough = _floor.footprint(floor, kind, R2, S)
        return {"cells": cells, "resolution": self.voxel, "axes": (u, v),
                "origin": (float(self.lo[u] - 0.5 * self.voxel), float(self.lo[v] - 0.5 * self.voxel)),
                "floor": floor, "floor_height": _floor.floor_heights(floor, self.lo[a], self.voxel, sign), "kind": kind,
                "why": why, "rough": rough, "up_axis": a, "up_sign": sign}

    def _radius_d2(self, robot_radius, what):
        """floor((robot_radius / voxel)^2), the squared lattice distance a passable cell must exceed; ValueError for a
        radius outside the field's band (slice_arguments' rule)."""
        robot_radius = float(robot_radius)
        if not 0 <= robot_radius <= self.radius_voxels * self.voxel:
            raise ValueError(f"{what}: robot_radius {robot_radius} m outside [0, {self.radius_voxels * self.voxel}], "
                             "the band of this field (build it with a larger max_distance)")
        return int(math.floor((robot_radius / self.voxel) ** 2))

    @torch.no_grad()
    def passable(self, robot_radius=0.0, allow_unknown=False):
        """uint8 [nx,ny,nz]: 1 where the centre of a robot of `robot_radius` metres may be -- the point was seen free
        (with `allow_unknown`: was not seen solid) and its squared distance to the nearest site exceeds
        floor((robot_radius / voxel)^2): the complement of `occupancy_slice`'s occupied rule.  Elementwise torch, once
        per plan.  ValueError for a radius beyond the field's band."""
        occ_d2 = self._radius_d2(robot_radius, "ESDF.passable")
        seen = (self.state != 2) if allow_unknown else (self.state == 1)
        return (seen & (self.d2 > occ_d2)).to(torch.uint8)

    def plan_arguments(self, points, robot_radius=0.0, snap=0.0, max_cost_m=None, what="ESDF.plan"):
        """(nearest lattice cells of the world `points`, snap radius in cells, max_cost in milli-voxels or None) for
        `plan` and `reachable`, or ValueError: a point that is no three finite numbers, a radius beyond the band, a
        negative snap, a point whose cell lies outside the lattice while snap is 0, a max_cost_m that is not positive
        or beyond 0x3fffffff - 1732 milli-voxels.  Touches no device."""
        self._radius_d2(robot_radius, what)
        snap = float(snap)
        if not (snap >= 0 and math.isfinite(snap)):
            raise ValueError(f"{what}: snap must be a finite distance >= 0 in metres (got {snap})")
        max_cost = None
        if max_cost_m is not None:
            max_cost_m = float(max_cost_m)
            if not (max_cost_m > 0 and max_cost_m / self.voxel * 1000.0 <= _plan.MAX_COST):
                raise ValueError(f"{what}: max_cost_m must be positive and at most "
                                 f"{_plan.MAX_COST * self.voxel / 1000.0} m on this lattice (got {max_cost_m})")
            max_cost = int(math.floor(max_cost_m / self.voxel * 1000.0))
        cells = []
        for p in points:
            try:
                xyz = [float(v) for v in (p.tolist() if hasattr(p, "tolist") else p)]
            except (TypeError, ValueError):
                xyz = []
            if len(xyz) != 3 or not all(math.isfinite(v) for v in xyz):
                raise ValueError(f"{what}: a point is three finite world coordinates (got {p!r})")
            cell = [int(math.floor((xyz[a] - self.lo[a]) / self.voxel + 0.5)) for a in range(3)]
            if snap == 0 and not all(0 <= cell[a] < self.dims[a] for a in range(3)):
                raise ValueError(f"{what}: point {xyz} is lattice point {cell}, outside the lattice {self.dims} "
                                 "(snap > 0 moves an endpoint to the nearest passable cell)")
            cells.append(cell)
        return cells, snap / self.voxel, max_cost

    def _no_route(self, start_cell, goal_cell, sweeps):
        """`plan`'s dict in its unreachable shape."""
        return {"reachable": False, "cells": torch.zeros((0, 3), dtype=torch.int32, device=self.device),
                "points": torch.zeros((0, 3), dtype=torch.float64, device=self.device), "length_m": math.inf,
                "min_clearance_m": math.nan, "start_cell": start_cell, "goal_cell": goal_cell, "sweeps": sweeps}

    def _route(self, cells):
        """(points float64 [L,3], the world coordinates of the lattice `cells` [L,3]; the smallest `dist` over them, a
        0-d tensor): both stay on the device."""
        idx = cells.long()
        lo = torch.tensor(self.lo, dtype=torch.float64, device=self.device)
        return lo[None, :] + cells.double() * self.voxel, self.dist[idx[:, 0], idx[:, 1], idx[:, 2]].min()

    @torch.no_grad()
    def _waypoints(self, route, passable, straighten, window):
        """`route` as it is without `straighten`, else with the keys of `plan.with_waypoints` over `passable`."""
        if not straighten:
            return route
        lo = torch.tensor(self.lo, dtype=torch.float64, device=self.device)[None, :]
        return _plan.with_waypoints(route, passable, window, lambda c: lo + c.double() * self.voxel, self.voxel, self.d2,
                                    self.dist, "ESDF.straighten")

    @torch.no_grad()
    def straighten(self, route, robot_radius=0.0, allow_unknown=False, window=_plan.DEFAULT_WINDOW):
        """The dict `route` of `plan`, `explore` or `next_view` (not changed) with its straightened form added: the
        shortest route over the path's own cells whose straight legs a robot of `robot_radius` may take
        (plan.straighten over `passable(robot_radius, allow_unknown)`: give the radius the route was planned with, each
        cell is tested against the `window` cells before it).  New keys: "waypoint_index" int32 [K], the kept cells'
        positions in "cells", first and last always among them, "waypoints" int32 [K,3], "waypoint_points" float64 [K,3]
        world coordinates, "straight_length_m" <= length_m, and "straight_min_clearance_m": `dist` at the cell with the
        smallest d2 that the straight legs cross (gs_segment_min), so it rounds as min_clearance_m does.  An unreachable
        route gets empty waypoints, inf and nan.  ValueError before the device is touched; RuntimeError when the route
        does not pass over `passable` (another radius than it was planned with)."""
        what = "ESDF.straighten"
        self._radius_d2(robot_radius, what)
        _plan._window(window, what)
        if not isinstance(route, dict) or "cells" not in route:
            raise ValueError(f"{what}: route is the dict of ESDF.plan, explore or next_view")
        return self._waypoints(route, self.passable(robot_radius, allow_unknown), True, window)

    @torch.no_grad()
    def sees(self, a_world, b_world, robot_radius=0.0, allow_unknown=False):
        """bool [n] on the device: whether a robot of `robot_radius` may go straight from the world point a_world[i] to
        b_world[i] ([n,3], or one point each: then one bool [1]) -- plan.line_of_sight between the points' nearest
        lattice points over `passable(robot_radius, allow_unknown)`.  A point outside the lattice sees nothing.
        ValueError for points that are no finite [n,3] or a radius beyond the band, before the device is touched."""
        what = "ESDF.sees"
        self._radius_d2(robot_radius, what)
        ends = []
        for name, p in (("a_world", a_world), ("b_world", b_world)):
            p = p.detach().cpu().numpy() if isinstance(p, torch.Tensor) else p
            try:
                p = np.asarray(p, dtype=np.float64)
            except (TypeError, ValueError):
                raise ValueError(f"{what}: {name} must be world points [n,3] (got {p!r})") from None
            p = p.reshape(1, 3) if p.shape == (3,) else p
            if p.ndim != 2 or p.shape[1] != 3 or not np.isfinite(p).all():
                raise ValueError(f"{what}: {name} must be finite world points [n,3] (got shape {list(p.shape)})")
            cell = np.floor((p - self.lo[None, :]) / self.voxel + 0.5)
            ends.append(np.clip(cell, -1, MAX_POINTS).astype(np.int32))      # outside stays outside
        if ends[0].shape != ends[1].shape:
            raise ValueError(f"{what}: a_world is {list(ends[0].shape)} and b_world is {list(ends[1].shape)}")
        return _plan.line_of_sight(self.passable(robot_radius, allow_unknown), ends[0], ends[1])

    @torch.no_grad()
    def plan(self, start, goal, robot_radius=0.0, allow_unknown=False, snap=0.0, max_cost_m=None, straighten=False,
             window=_plan.DEFAULT_WINDOW):
        """The shortest collision-free route of a robot of `robot_radius` from the world point `start` to `goal` over
        the lattice (plan.geodesic_field seeded at the goal, GeodesicField.path from the start).  A point maps to its
        nearest lattice point; with `snap` > 0 metres an endpoint whose cell does not pass moves to the passable cell
        at the smallest squared lattice distance within `snap`, ties to the lowest linear index (camera centres
        usually sit in never-observed cells).  Routes longer than `max_cost_m` count as unreachable.  -> {"reachable",
        "cells": int32 [L,3] on the device, "points": float64 [L,3] world coordinates start to goal, "length_m":
        cost[start] * voxel / 1000, "min_clearance_m": the smallest `dist` over the path's cells, "start_cell",
        "goal_cell" (None when no passable cell was found), "sweeps"}; unreachable: L = 0, length_m inf,
        min_clearance_m nan.  With `straighten` the dict gains the keys of `ESDF.straighten` (waypoint_index, waypoints,
        waypoint_points, straight_length_m, straight_min_clearance_m; window as there); without it nothing else is
        launched and the dict is the one above.  ValueError (plan_arguments; a bad window) before the device is
        touched."""
        (s, g), snap_cells, max_cost = self.plan_arguments([start, goal], robot_radius, snap, max_cost_m)
        _plan._window(window, "ESDF.plan")
        passable = self.passable(robot_radius, allow_unknown)
        s, g = _plan.snap_cell(passable, s, snap_cells), _plan.snap_cell(passable, g, snap_cells)
        out = self._no_route(s, g, 0)
        if s is None or g is None:
            return self._waypoints(out, passable, straighten, window)
        field = _plan.geodesic_field(passable, [g], max_cost)
        cells = field.path(s)
        out["sweeps"] = field.sweeps
        if int(cells.shape[0]) == 0:
            return self._waypoints(out, passable, straighten, window)
        points, clearance = self._route(cells)
        scalars = torch.stack([field.cost[s[0], s[1], s[2]].double(), clearance.double()]).cpu().tolist()   # one read
        out.update(reachable=True, cells=cells, points=points, length_m=scalars[0] * self.voxel / 1000.0,
                   min_clearance_m=scalars[1])
        return self._waypoints(out, passable, straighten, window)

    @torch.no_grad()
    def follow(self, start, goal, up_axis, heading=None, max_ticks=400, goal_tolerance=_follow.DEFAULT_TOLERANCE,
               **controller_args):
        """Drive a differential-drive base from the world point `start` to `goal` in the plane perpendicular to
        `up_axis` at `start`'s coordinate on it: `follow.Controller(self, goal, up_axis, height, **controller_args)` and
        its `drive` from `start` heading along `heading`, a direction (c, s) on the plane's two axes in increasing order
        (normalised here; default: down the cost-to-go field's first path step, (1, 0) where that step leaves the plane
        or there is none).  -> `Controller.drive`'s dict with "goal_cell" and "start_cell" added.  An unreachable goal
        gives reached False and empty traces with nothing launched beyond the field.  ValueError before the device is
        touched."""
        what = "ESDF.follow"
        robot_radius = controller_args.get("robot_radius", 0.0)
        (s_cell,), _, _ = self.plan_arguments([start], robot_radius, 0.0, None, what)
        if isinstance(up_axis, bool) or not isinstance(up_axis, (int, np.integer)) or not 0 <= int(up_axis) <= 2:
            raise ValueError(f"{what}: up_axis must be 0, 1 or 2 (got {up_axis!r})")
        if heading is not None:
            try:
                heading = [float(v) for v in heading]
            except (TypeError, ValueError):
                heading = []
            if len(heading) != 2 or not all(math.isfinite(v) for v in heading) or math.hypot(*heading) == 0:
                raise ValueError(f"{what}: heading is a direction (c, s) in the plane of motion (got {heading!r})")
        start = [float(v) for v in (start.tolist() if hasattr(start, "tolist") else start)]
        u, v = [ax for ax in range(3) if ax != int(up_axis)]
        controller_args.setdefault("robot_radius", robot_radius)
        ctl = _follow.Controller(self, goal, int(up_axis), start[int(up_axis)], **controller_args)
        if heading is None:
            heading = [1.0, 0.0]
            if ctl.goal_cell is not None:
                cells = ctl.field.path(s_cell, max_len=None)[:2].cpu().tolist()
                if len(cells) == 2 and (cells[1][u] != cells[0][u] or cells[1][v] != cells[0][v]):
                    heading = [float(cells[1][u] - cells[0][u]), float(cells[1][v] - cells[0][v])]
        norm = math.hypot(*heading)
        out = ctl.drive([start[u], start[v], heading[0] / norm, heading[1] / norm], max_ticks, goal_tolerance)
        out.update(goal_cell=ctl.goal_cell, start_cell=s_cell)
        return out

    @torch.no_grad()
    def reachable(self, seeds_world, robot_radius=0.0, allow_unknown=False, snap=0.0, max_cost_m=None):
        """bool [nx,ny,nz]: the cells a robot of `robot_radius` can reach from any of the world points `seeds_world`
        ([m,3], for example every camera centre), i.e. cost < INF of the field seeded at all of them.  Seeds are placed
        as `plan` places its endpoints; one without a passable cell is ignored."""
        seeds_world = seeds_world.detach().cpu().numpy() if isinstance(seeds_world, torch.Tensor) else seeds_world
        pts = np.asarray(seeds_world, dtype=np.float64)
        if pts.size == 0:
            pts = pts.reshape(0, 3)
        if pts.ndim != 2 or pts.shape[1] != 3:
            raise ValueError(f"ESDF.reachable: seeds_world must be [m,3] (got {list(pts.shape)})")
        cells, snap_cells, max_cost = self.plan_arguments(list(pts), robot_radius, snap, max_cost_m, "ESDF.reachable")
        passable = self.passable(robot_radius, allow_unknown)
        seeds = [c for c in (_plan.snap_cell(passable, c, snap_cells) for c in cells) if c is not None]
        field = _plan.geodesic_field(passable, np.array(seeds, dtype=np.int32).reshape(-1, 3), max_cost)
        return field.cost < _plan.INF

    @torch.no_grad()
    def frontiers(self, robot_radius=0.0, start=None, snap=0.0, max_cost_m=None, min_cells=1):
        """Where this field's free space ends in never-observed space: the `frontier.FrontierClusters` of `state` with
        `open` = `passable(robot_radius)`, the cells the robot's centre may be.  With `start` (a world point, placed like
        `plan`'s endpoints: its nearest lattice point, moved by `snap` to a passable cell) one `plan.geodesic_field`
        seeded at the start's cell prices every cluster; routes longer than `max_cost_m` count as none.  World-space
        extras on the result: `.centroid` float64 [K,3] = lo + centroid_cells * voxel, `.area_m2` float64 [K] = faces *
        voxel^2, `.cost_m` float64 [K] = best_cost * voxel / 1000, inf where INF, `.keep` bool [K] = size >= min_cells,
        `.start_cell` (None without a start or when no passable cell was found) and `.field` (the GeodesicField or
        None).  Host reads: those of `frontier_clusters` and of `geodesic_field`, and the small one of `snap_cell`.
        ValueError (plan_arguments; min_cells < 1) before the device is touched."""
        what = "ESDF.frontiers"
        cells, snap_cells, max_cost = self.plan_arguments([] if start is None else [start], robot_radius, snap,
                                                          max_cost_m, what)
        min_cells = _frontier._min_cells(min_cells, what)
        passable = self.passable(robot_radius)
        s = _plan.snap_cell(passable, cells[0], snap_cells) if cells else None
        field = None if s is None else _plan.geodesic_field(passable, [s], max_cost)
        out = _frontier.frontier_clusters(self.state, passable, None if field is None else field.cost)
        lo = torch.tensor(self.lo, dtype=torch.float64, device=out.device)
        out.centroid = lo[None, :] + out.centroid_cells() * self.voxel
        out.area_m2 = out.faces.double() * self.voxel ** 2
        out.cost_m = torch.where(out.best_cost >= _frontier.INF, math.inf, out.best_cost.double() * self.voxel / 1000.0)
        out.keep = out.size >= min_cells
        out.start_cell, out.field = s, field
        return out

    @torch.no_grad()
    def explore(self, start, robot_radius=0.0, snap=0.0, max_cost_m=None, min_cells=1, order="nearest", straighten=False,
                window=_plan.DEFAULT_WINDOW):
        """Where to go next from the world point `start` to see something new: `frontiers(...)`, then among the kept
        clusters a route leads to, `order` "nearest" takes the smallest best_cost, ties to the lowest root, "largest" the
        largest faces, then the smallest best_cost, then the lowest root; the route is the field's path from the
        cluster's best_cell, reversed so that it reads start to goal.  -> `plan`'s dict {"reachable", "cells", "points",
        "length_m", "min_clearance_m", "start_cell", "goal_cell", "sweeps" (the field's)} plus "cluster" (the id or
        None), "n_clusters", "n_kept", "n_reachable" and "clusters" (the FrontierClusters of `frontiers`); when no
        cluster qualifies, `plan`'s unreachable shape.  `straighten` and `window` as for `plan`.  One read of the table's
        columns besides those of `frontiers` and `plan`."""
        if order not in _frontier.ORDERS:
            raise ValueError(f"ESDF.explore: order must be one of {_frontier.ORDERS} (got {order!r})")
        _plan._window(window, "ESDF.explore")
        out = self._explore(start, robot_radius, snap, max_cost_m, min_cells, order)
        return self._waypoints(out, self.passable(robot_radius), True, window) if straighten else out

    def _explore(self, start, robot_radius, snap, max_cost_m, min_cells, order):
        """`explore`'s route."""
        self.plan_arguments([start], robot_radius, snap, max_cost_m, "ESDF.explore")      # a start is needed here
        fc = self.frontiers(robot_radius, start, snap, max_cost_m, min_cells)
        out = dict(self._no_route(fc.start_cell, None, 0 if fc.field is None else fc.field.sweeps), cluster=None,
                   n_clusters=fc.n_clusters, n_kept=0, n_reachable=0, clusters=fc)
        if fc.n_clusters == 0:
            return out
        cols = torch.stack([fc.best_cost.long(), fc.faces.long(), fc.root.long(), fc.keep.long(),
                            fc.best_cell.long()]).cpu().tolist()                                        # one read
        best_cost, faces, root, keep, best_cell = cols
        out["n_kept"] = sum(keep)
        out["n_reachable"] = sum(1 for k, c in zip(keep, best_cost) if k and c < _frontier.INF)
        row = _frontier.choose(best_cost, faces, root, keep, order)
        if row is None or fc.field is None:
            return out
        n1, n2 = self.dims[1], self.dims[2]
        goal = [best_cell[row] // (n1 * n2), best_cell[row] // n2 % n1, best_cell[row] % n2]
        cells = torch.flip(fc.field.path(goal), dims=[0]).contiguous()
        if int(cells.shape[0]) == 0:
            return out
        points, clearance = self._route(cells)
        out.update(reachable=True, cells=cells, points=points, length_m=best_cost[row] * self.voxel / 1000.0,
                   min_clearance_m=float(clearance.item()), goal_cell=goal, cluster=row)
        return out

    def rooms_arguments(self, robot_radius=0.0, core_radius=0.6, min_core_m3=None, min_core_cells=None, max_cost_m=None):
        """(min_core_cells, max_cost in milli-voxels or None) of `rooms`, or ValueError: radii that are not robot_radius <
        core_radius <= the field's band, a min_core_m3 that is not positive and finite, a min_core_cells that is no
        positive integer, both of them given, a max_cost_m out of range (plan_arguments).  Touches no device."""
        what = "ESDF.rooms"
        _, _, max_cost = self.plan_arguments([], robot_radius, 0.0, max_cost_m, what)
        core_radius = float(core_radius)
        band = self.radius_voxels * self.voxel
        if not float(robot_radius) < core_radius <= band:
            raise ValueError(f"{what}: need robot_radius < core_radius <= {band} m, the band of this field (got "
                             f"{float(robot_radius)} and {core_radius}; build the field with a larger max_distance)")
        if min_core_m3 is not None and min_core_cells is not None:
            raise ValueError(f"{what}: give min_core_m3 or min_core_cells, not both")
        if min_core_m3 is not None:
            min_core_m3 = float(min_core_m3)
            if not (min_core_m3 > 0 and math.isfinite(min_core_m3)):
                raise ValueError(f"{what}: min_core_m3 must be positive and finite (got {min_core_m3})")
            min_core_cells = max(int(math.ceil(min_core_m3 / self.voxel ** 3)), 1)
        elif min_core_cells is None:
            min_core_cells = 1
        elif isinstance(min_core_cells, bool) or not isinstance(min_core_cells, (int, np.integer)) or \
                int(min_core_cells) < 1:
            raise ValueError(f"{what}: min_core_cells must be a positive integer (got {min_core_cells!r})")
        return int(min_core_cells), max_cost

    @torch.no_grad()
    def rooms(self, robot_radius=0.0, core_radius=0.6, min_core_m3=None, min_core_cells=None, allow_unknown=False,
              max_cost_m=None):
        """Which rooms this field's free space has and which doorways join them: the `rooms.RoomSegments` of `open` =
        `passable(robot_radius, allow_unknown)`, `core` = `passable(core_radius)` and `d2`.  A place where a ball of
        `core_radius` fits is the inside of a room; its connected pieces of at least `min_core_cells` cells (or
        `min_core_m3` cubic metres; default: one cell) seed a room each, and every cell the robot can be at joins the
        seed it is nearest to along a route, routes longer than `max_cost_m` counting as none.  World-space extras on the
        result: `.lo`, `.voxel`, `.centroid` float64 [K,3] = lo + centroid_cells * voxel, `.volume_m3` float64 [K] = size *
        voxel^3, `.box_lo` / `.box_hi` float64 [K,3], the corners of every room's box, and per doorway `.door_centre`
        float64 [D,3], its widest cell (where a robot passes), `.door_width_m` float64 [D] = 2 * sqrt(widest_d2) * voxel
        (between the lattice points at the jambs: up to two voxels below the clear opening) and `.door_centroid` float64
        [D,3].  Host reads: those of `rooms.room_segments`.  ValueError (rooms_arguments)
        before the device is touched."""
        min_core_cells, max_cost = self.rooms_arguments(robot_radius, core_radius, min_core_m3, min_core_cells, max_cost_m)
        out = _rooms.room_segments(self.passable(robot_radius, allow_unknown), self.passable(core_radius), self.d2,
                                   min_core_cells, max_cost)
        lo = torch.tensor(self.lo, dtype=torch.float64, device=out.device)[None, :]
        out.lo, out.voxel = self.lo, self.voxel
        out.centroid = lo + out.centroid_cells() * self.voxel
        out.volume_m3 = out.rooms["size"].double() * self.voxel ** 3
        out.box_lo = lo + out.rooms["bbox"][:, :3].double() * self.voxel
        out.box_hi = lo + out.rooms["bbox"][:, 3:].double() * self.voxel
        w = out.doors["widest_cell"].long()
        n1, n2 = self.dims[1], self.dims[2]
        out.door_centre = lo + torch.stack([w // (n1 * n2), w // n2 % n1, w % n2], dim=1).double() * self.voxel
        out.door_width_m = 2.0 * torch.sqrt(out.doors["widest_d2"].double()) * self.voxel
        out.door_centroid = lo + out.centroid_cells(out.doors) * self.voxel
        return out

    def view_candidates(self, start, up_axis, height, robot_radius=0.0, stride=4, snap=0.0, max_cost_m=None,
                        max_candidates=4096):
        """Where a robot of `robot_radius` could stand to look around: (cells int32 [V,3], cost int32 [V] in milli-voxels,
        the GeodesicField), on the device.  A candidate is a passable cell with a route from the world point `start`
        (placed as `plan` places its endpoints) of at most `max_cost_m`, on a layer of `up_axis` inside `height` (h0, h1)
        metres by `slice_arguments`' rule, whose two other coordinates are multiples of `stride`; they come by ascending
        (cost, linear index), the first `max_candidates` of them.  torch ops and one `plan.geodesic_field`; no candidates
        and a field of None when the start has no passable cell.  ValueError before the device is touched."""
        return _view.esdf_view_candidates(self, start, up_axis, height, robot_radius, stride, snap, max_cost_m,
                                          max_candidates)

    def next_view(self, start, camera, up_axis, height, n_yaw=8, robot_radius=0.0, stride=4, snap=0.0, max_cost_m=None,
                  max_candidates=4096, max_unknown=0, min_gain_cells=1, min_solid_cells=0, lam=0.0, straighten=False,
                  window=_plan.DEFAULT_WINDOW):
        """Where to stand, which way to look and how much of the unknown would be seen from there: the `view_candidates`,
        each looked from at the `n_yaw` headings 2 pi j / n_yaw about `up_axis` with `camera` = {hfov_deg, vfov_deg, n_u,
        n_v, range_m, pitch_deg} (view.ray_directions; range_m / voxel rounded down to cells) -- one gs_view_gain call per
        heading, each with its own tight box (view.view_gain) -- then one read of the [V, n_yaw, 4] table and the costs
        and the choice on the host (view.choose): among the (view, heading) pairs with unknown >= `min_gain_cells` and
        solid >= `min_solid_cells` the largest unknown * voxel^3 * exp(-lam * cost_m) wins, equal scores going to the
        lower cost, then the lower linear index, then the lower heading.  -> `plan`'s dict, the route start to view, plus
        "view_cell", "view_point", "yaw", "yaw_index", "gain_cells", "gain_m3", "free_cells", "solid_cells", "score",
        "n_candidates", "n_qualified" and "gains" (the device table); when nothing qualifies, `plan`'s unreachable shape
        with "view_cell" None.  `straighten` and `window` as for `plan`.  ValueError before the device is touched."""
        _plan._window(window, "ESDF.next_view")
        out = _view.esdf_next_view(self, start, camera, up_axis, height, n_yaw, robot_radius, stride, snap, max_cost_m,
                                   max_candidates, max_unknown, min_gain_cells, min_solid_cells, lam)
        return self._waypoints(out, self.passable(robot_radius), True, window) if straighten else out

    def save_map(self, directory, up_axis, height, robot_radius=0.0, known_fraction=0.5):
        """`occupancy_slice` written as `directory`/occupancy.pgm and occupancy.yaml (save_map); returns the slice."""
        grid = self.occupancy_slice(up_axis, height, robot_radius, known_fraction)
        save_map(directory, grid)
        return grid


def save_map(directory, grid):
    """Write `ESDF.occupancy_slice`'s dict as a ROS map_server map: occupancy.pgm (binary P5, n_u wide, n_v high; file
    row r is image index v = n_v - 1 - r, the column is u, so the picture has u to the right and v upward) and
    occupancy.yaml with the keys image, resolution, origin [x, y, 0.0], negate 0, occupied_thresh 0.65, free_thresh 0.196.
    Numbers are written with repr(): `load_map` gives them back bit for bit."""
    cells = grid["cells"]
    cells = cells.detach().cpu().numpy() if isinstance(cells, torch.Tensor) else np.asarray(cells)
    if cells.ndim != 2 or cells.dtype != np.uint8:
        raise ValueError(f"save_map: cells must be uint8 [n_u,n_v] (got {cells.dtype} {list(cells.shape)})")
    n_u, n_v = cells.shape
    os.makedirs(directory, exist_ok=True)
    with open(os.path.join(directory, "occupancy.pgm"), "wb") as fh:
        fh.write(f"P5\n{n_u} {n_v}\n255\n".encode("ascii"))
        fh.write(np.ascontiguousarray(cells[:, ::-1].T).tobytes())
    x, y = (float(c) for c in grid["origin"])
    with open(os.path.join(directory, "occupancy.yaml"), "w") as fh:
        fh.write(f"image: occupancy.pgm\nresolution: {float(grid['resolution'])!r}\norigin: [{x!r}, {y!r}, 0.0]\n"
                 "negate: 0\noccupied_thresh: 0.65\nfree_thresh: 0.196\n")


def load_map(directory):
    """save_map's inverse: {"cells": uint8 [n_u,n_v] (host), "origin": (x, y), "resolution"}."""
    keys = {}
    with open(os.path.join(directory, "occupancy.yaml")) as fh:
        for line in fh:
            name, _, value = line.partition(":")
            keys[name.strip()] = value.strip()
    origin = [float(c) for c in keys["origin"].strip("[]").split(",")]
    with open(os.path.join(directory, keys["image"]), "rb") as fh:
        data = fh.read()
    magic, size, maxval, pixels = data.split(b"\n", 3)
    n_u, n_v = (int(s) for s in size.split())
    if magic != b"P5" or maxval != b"255" or len(pixels) != n_u * n_v:
        raise ValueError(f"load_map: {directory}/{keys['image']} is not an 8-bit binary PGM of the size it names")
    rows = np.frombuffer(pixels, dtype=np.uint8).reshape(n_v, n_u)
    return {"cells": np.ascontiguousarray(rows.T[:, ::-1]), "origin": (origin[0], origin[1]),
            "resolution": float(keys["resolution"])}


CLEARANCE_REPORT_ORDER = ("clearance_min_m", "clearance_mean_m", "n_inside", "n_unknown", "n_poses")


def clearance_text(result):
    """The text of metrics_tsdf_clearance.txt: two header lines, then `name<TAB>value` per reported value, written
    with repr() so that reading the file gives back the numbers bit for bit."""
    lines = ["Clearance of the estimated camera centres in the fused TSDF volume's distance field: the distance [m] to "
             "the nearest surface, over the centres that lie in a cell whose eight corners were seen",
             "(n_inside: such centres with a negative distance, inside fused solid; n_unknown: centres outside the "
             "lattice or in a cell with a never-seen corner; nan without any usable centre)"]
    lines += [f"{k}\t{result[k]!r}" for k in CLEARANCE_REPORT_ORDER]
    return "\n".join(lines) + "\n"


def parse_clearance(text):
    """clearance_text's inverse: the reported dict."""
    lines = text.splitlines()
    if len(lines) != 2 + len(CLEARANCE_REPORT_ORDER) or not lines[0].startswith("Clearance of the estimated camera"):
        raise ValueError("not a metrics_tsdf_clearance.txt")
    result = {}
    for key, line in zip(CLEARANCE_REPORT_ORDER, lines[2:]):
        name, value = line.split("\t")
        if name != key:
            raise ValueError(f"metrics_tsdf_clearance.txt: expected {key}, found {name}")
        result[key] = int(value) if key.startswith("n_") else float(value)
    return result


@torch.no_grad()
def trajectory_clearance(esdf, c2w_list, out_path=None):
    """Query `esdf` at the camera centres of the camera-to-world poses c2w_list ([4,4] or [3,4] each, the volume's
    frame).  -> {"clearance_min_m", "clearance_mean_m": over the valid and known centres (nan without one), "n_inside":
    known centres with dist < 0, "n_unknown": invalid or not known ones, "n_poses"}; the sums are fp64 on the device and
    read back in one read.  With `out_path` also writes clearance_text() there."""
    n = len(c2w_list)
    centres = torch.stack([torch.as_tensor(c)[:3, 3] for c in c2w_list]).to(torch.float32) if n else torch.zeros(0, 3)
    res = esdf.query(centres)
    ok = res["valid"] & res["known"]
    d = res["dist"].double()
    inf = torch.full_like(d, math.inf)
    sums = torch.stack([torch.where(ok, d, inf).min() if n else inf.sum(), (d * ok).sum(), ok.sum().double(),
                        (ok & (res["dist"] < 0)).sum().double()]).cpu().tolist()             # the one read
    n_ok = int(sums[2])
    result = {"clearance_min_m": sums[0] if n_ok else math.nan, "clearance_mean_m": sums[1] / n_ok if n_ok else math.nan,
              "n_inside": int(sums[3]), "n_unknown": n - n_ok, "n_poses": n}
    if out_path is not None:
        with open(out_path, "w") as fh:
            fh.write(clearance_text(result))
    return result


def _inverse(disp):
    return torch.where(disp > 0, 1.0 / disp, torch.zeros_like(disp))


@torch.no_grad()
def keyframe_observations(video, source, ids, intr, w2w_inv, filter_thresh=0.01, visible_num=2, depth_filter=None):
    """What `fuse_keyframes` fuses for the keyframes `ids` (int64, host) of one chunk, as its docstring says per source:
    (depth [k,H,W], w2c [k,7], images [k,3,H,W], mask [k,H,W] or None).  `intr` is intrinsics[0] * 8 on the device,
    `w2w_inv` SE3(pose_compensate[0]).inv().  `depth_filter`: the count behind the "tracked" mask, droid_backends' by
    default (tests pass their restatement's).  `tsdf_live.LiveFusion` fuses through the same rule."""
    if depth_filter is None:
        from . import droid_backends
        depth_filter = droid_backends.depth_filter
    dev = video.disps_up.device
    poses = video.poses_filtered if source == "filtered" else video.poses
    ids_d = ids.to(dev)
    w2c = (SE3(poses[ids_d]) * w2w_inv).data       # the inverse of w2w * SE3(pose).inv(); exact for the identity
    mask = None
    if source == "tracked":
        disps = _rows(video.disps_up, ids)
        thresh = float(filter_thresh) * torch.ones(ids.numel(), dtype=torch.float32, device=dev)
        count = depth_filter(video.poses, video.disps_up, intr, ids_d, thresh)
        mask = ((count >= visible_num) & (disps > 0.01 * disps.mean(dim=[1, 2], keepdim=True))).float()
        depth = _inverse(disps)
    elif source == "filtered":
        depth = _inverse(_rows(video.disps_filtered, ids))
        mask = _rows(video.mask_filtered, ids)
    else:
        depth = _rows(video.depths_gt, ids)
    return depth, w2c, _rows(video.images, ids), mask


def _sensor_needs_rgbd(video, what):
    if getattr(video, "cfg", None) is not None and video.cfg.get("mode", "rgbd") != "rgbd":
        raise ValueError(f"{what}: source='sensor' needs rgbd mode (mode is {video.cfg.get('mode')!r}: "
                         "no sensor depth is stored)")


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
    dev = video.disps_up.device
    num = int(video.disps_up.shape[0])
    if source in ("tracked", "sensor"):
        if source == "sensor":
            _sensor_needs_rgbd(video, "fuse_keyframes")
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
    for a in range(0, idx.numel(), CHUNK):
        depth, w2c, images, mask = keyframe_observations(video, source, idx[a:a + CHUNK], intr, w2w_inv, filter_thresh,
                                                         visible_num)
        vol.integrate(depth, w2c, intr_host, images=images, mask=mask)
    return vol, vol.extract_mesh(min_weight)


DEPTH_REPORT_ORDER = ("depth_l1_cm", "coverage", "n_frames")     # order of the lines of metrics_tsdf_depth.txt
EVAL_CHUNK = 16                                                  # frames per raycast in eval_tsdf_depth


def depth_metrics_text(result, frames, per_frame, metric_depth=True):
    """The text of metrics_tsdf_depth.txt: two header lines, `name<TAB>value` per reported value, then one line per
    evaluated frame, `index depth_l1 coverage n_depth` (depth_l1 in m).  Values are written with repr(): reading the file
    gives back the fp64 numbers bit for bit."""
    why = "depth L1 over the pixels with a hit and sensor depth > 0" if metric_depth else \
        "nan and no frames: without sensor depth (mode is not rgbd) there is nothing metric to compare with"
    lines = ["Raycast of the TSDF volume against the sensor depth: depth L1 (first zero crossing along each pixel's ray, "
             "depth along the optical axis), coverage (share of the pixels with sensor depth that have a hit)",
             f"(means over the evaluated frames; {why}; then per frame: index depth_l1[m] coverage n_depth)"]
    lines += [f"{k}\t{result[k]!r}" for k in DEPTH_REPORT_ORDER]
    rows = np.asarray(per_frame, dtype=np.float64).reshape(len(frames), 4)
    lines += [f"{int(i)} {float(r[0])!r} {float(r[1])!r} {int(r[2])}" for i, r in zip(frames, rows)]
    return "\n".join(lines) + "\n"


def parse_depth_metrics(text):
    """depth_metrics_text's inverse: (reported dict, [(index, depth_l1, coverage, n_depth), ...])."""
    lines = text.splitlines()
    if len(lines) < 2 + len(DEPTH_REPORT_ORDER) or not lines[0].startswith("Raycast of the TSDF volume"):
        raise ValueError("not a metrics_tsdf_depth.txt")
    result = {}
    for key, line in zip(DEPTH_REPORT_ORDER, lines[2:]):
        name, value = line.split("\t")
        if name != key:
            raise ValueError(f"metrics_tsdf_depth.txt: expected {key}, found {name}")
        result[key] = int(value) if key == "n_frames" else float(value)
    frames = []
    for line in lines[2 + len(DEPTH_REPORT_ORDER):]:
        i, d, c, n = line.split(" ")
        frames.append((int(i), float(d), float(c), int(n)))
    return result, frames


def summarize_depth(frames, per_frame):
    """frames: the evaluated indices; per_frame: host fp64 [F,4] (depth_l1 in m, coverage, n_depth, n_valid).  -> the
    reported dict: the mean depth_l1 in cm over the frames with a compared pixel, the mean coverage over the frames with
    sensor depth, and n_frames."""
    from .neus.render_eval import frame_mean
    rows = np.asarray(per_frame, dtype=np.float64).reshape(len(frames), 4)
    return {"depth_l1_cm": 100.0 * frame_mean([r[0] for r in rows if r[2] > 0]),
            "coverage": frame_mean([r[1] for r in rows if r[3] > 0]), "n_frames": len(frames)}


@torch.no_grad()
def eval_tsdf_depth(vol, stream, c2w_list, intrinsics, every=5, out_path=None, save_images=False, step=0.5,
                    min_weight=1.0, metric_depth=True, return_images=False):
    """Raycast `vol` at every `every`-th frame of `stream` from its camera-to-world pose c2w_list[i] ([4,4] or [3,4], the
    volume's frame: what terminate holds as estimate_c2w_list) and compare the depth image with the frame's sensor
    depth.  Per frame: depth_l1 [m] over the pixels with both a hit and sensor depth > 0, n_depth their number, coverage
    = n_depth / the number of pixels with sensor depth.  The sums are fp64 on the device, kept in one [F,4] tensor and
    read once.  Returns summarize_depth()'s dict plus `frames` and `per_frame` (host fp64 [F,4]: depth_l1, coverage,
    n_depth, n_valid), with `return_images` also `depth` and `hit` ([F,H,W], on the device); with `out_path` writes that
    file, with `save_images` also tsdf_eval/{i:05d}.jpg beside it: the normal map as (n + 1) / 2 | the input frame.
    metric_depth=False (the run had no sensor depth): nothing is raycast, the file says why and holds nan."""
    every = int(every)
    if every < 1:
        raise ValueError("eval_tsdf_depth: every must be at least 1")
    if save_images and out_path is None:
        raise ValueError("eval_tsdf_depth: save_images needs out_path (the images go beside it)")
    dev = vol.device
    img_dir = None
    if save_images and metric_depth:
        img_dir = os.path.join(os.path.dirname(os.path.abspath(out_path)), "tsdf_eval")
        os.makedirs(img_dir, exist_ok=True)
    frames = list(range(0, len(stream), every)) if metric_depth else []
    rows, depths = [], []
    for a in range(0, len(frames), EVAL_CHUNK):
        ids = frames[a:a + EVAL_CHUNK]
        items = [stream[i] for i in ids]
        gt = torch.stack([it[2].to(dev, torch.float32) for it in items])
        c2w = torch.stack([torch.as_tensor(c2w_list[i])[:3, :] for i in ids]).to(torch.float32)
        out = vol._raycast(c2w, intrinsics, tuple(gt.shape[1:]), step=step, min_weight=min_weight,
                           color=False)
        pred = out["depth"]
        valid = gt > 0
        both = valid & (pred > 0)
        n_valid, n_depth = valid.sum(dim=(1, 2)).double(), both.sum(dim=(1, 2)).double()
        l1 = ((pred.double() - gt.double()).abs() * both).sum(dim=(1, 2)) / n_depth
        rows.append(torch.stack([l1, n_depth / n_valid, n_depth, n_valid], dim=1))
        if return_images:
            depths.append(pred)
        if img_dir is not None:
            from .neus.render_eval import _interleaved, _save_side_by_side
            for j, i in enumerate(ids):
                colour = _interleaved(items[j][1], "the stream's colour").to(dev, torch.float32)
                _save_side_by_side(os.path.join(img_dir, f"{i:05d}.jpg"), (out["normal"][j] + 1.0) * 0.5, colour)
    per_frame = (torch.cat(rows) if rows else torch.zeros(0, 4, dtype=torch.float64)).cpu().numpy()      # the one read
    result = summarize_depth(frames, per_frame)
    if out_path is not None:
        with open(out_path, "w") as fh:
            fh.write(depth_metrics_text(result, frames, per_frame, metric_depth=metric_depth))
    result.update(frames=frames, per_frame=per_frame)
    if return_images:
        result["depth"] = torch.cat(depths) if depths else torch.zeros(0, 0, 0, device=dev)
        result["hit"] = result["depth"] > 0
    return result


def fuse_from_config(slam, stream=None, trans_init=None, c2w_list=None, stats=None):
    """`SLAM.terminate`'s TSDF step, `tsdf_run.fuse_from_config` (which imports this module: hence not at the top)."""
    from .tsdf_run import fuse_from_config as run
    return run(slam, stream=stream, trans_init=trans_init, c2w_list=c2w_list, stats=stats)
