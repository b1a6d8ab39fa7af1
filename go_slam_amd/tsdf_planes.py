"""The dominant planes of a `TSDFVolume`, the floor among them and the volume stood upright on it.

The navigation keys (`ESDF.occupancy_slice`, `plan`, `frontiers`, `next_view`) take an `up_axis` and a `height` interval:
they assume that one lattice axis is vertical.  A run's world frame is its first camera's, and a hand-held first frame is
tilted.  This module finds the planes a fused volume holds, picks the floor by a stated policy and resamples the volume
into a frame whose `up_axis` is the floor's normal and whose coordinate 0 along it is the floor.

csrc/tsdf_planes.hip has the three kernels, which share one surface sample per cell of the lattice: gs_tsdf_plane_votes
(a cube-map histogram of the samples' normal directions), gs_tsdf_plane_offsets (for given directions, histograms of the
samples' offsets along them) and gs_tsdf_plane_moments (for given planes, the fp64 moments of the samples within a band,
in tsdf_align.hip's fixed summation order).  Arithmetic contract: include/goslam_hip.h (gs_tsdf_plane_*);
tests/tsdf_planes_restatement.py restates it.

Everything between the kernels is fp64 NumPy on the host and takes the kernels through a `field`: an object with `dims`,
`lo`, `voxel` and the methods `votes`, `offsets` and `moments`.  `DeviceField` is the one over a volume on the GPU; the
restatement brings its own, so `find_planes_in` is one code for both.

`find_planes` (TSDFVolume.find_planes) returns the planes, `floor_plane` picks the floor, `upright_transform` makes the
rigid transform world to map, `upright_volume` (TSDFVolume.upright) resamples, and `planes_text` / `parse_planes` write and
read metrics_tsdf_planes.txt (tsdf.fuse_from_config, cfg["tsdf"]["planes"] and cfg["tsdf"]["upright"]).
"""
import math

import numpy as np

from . import _lib
from . import tsdf_merge as _merge

MAX_PLANES = 16                                  # planes or directions of one kernel call
MAX_OFFSET_BINS = 2048
MEAN_SHIFT_ROUNDS = 32
WALL_DEG = 10.0                                  # heading="walls": how far from perpendicular to the floor a wall may be


# ---- arguments ----------------------------------------------------------------------------------------------------------
def _vector3(v, what, name):
    try:
        v = np.asarray(v, np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: {name} must be three numbers") from None
    if v.shape != (3,) or not np.isfinite(v).all() or not np.linalg.norm(v) > 0:
        raise ValueError(f"{what}: {name} must be three finite numbers, not all zero (got {v.tolist()})")
    return v / np.linalg.norm(v)


def find_arguments(what, voxel, bins=16, cone_deg=10.0, band=None, max_planes=8, min_cells=64, min_weight=1.0, iterations=3):
    """The checked arguments of `find_planes`: a dict; cos2, band and min_weight are rounded to fp32 here, as the kernels
    take them.  ValueError otherwise."""
    if int(bins) != bins or not 2 <= int(bins) <= 64 or int(bins) % 2:
        raise ValueError(f"{what}: bins must be an even number in [2, 64] (got {bins})")
    cone_deg = float(cone_deg)
    if not 0 < cone_deg < 90:
        raise ValueError(f"{what}: cone_deg must lie in (0, 90) (got {cone_deg})")
    band = float(voxel) if band is None else float(band)
    if not (band > 0 and math.isfinite(band)):
        raise ValueError(f"{what}: band must be positive and finite, in metres (got {band})")
    if int(max_planes) != max_planes or not 1 <= int(max_planes) <= MAX_PLANES:
        raise ValueError(f"{what}: max_planes must lie in [1, {MAX_PLANES}] (got {max_planes})")
    if int(min_cells) != min_cells or int(min_cells) < 1:
        raise ValueError(f"{what}: min_cells must be at least 1 (got {min_cells})")
    min_weight = float(min_weight)
    if not math.isfinite(min_weight):
        raise ValueError(f"{what}: min_weight must be finite (got {min_weight})")
    if int(iterations) != iterations or int(iterations) < 0:
        raise ValueError(f"{what}: iterations must be at least 0 (got {iterations})")
    return {"bins": int(bins), "cone_deg": cone_deg, "cos2": float(np.float32(math.cos(math.radians(cone_deg)) ** 2)),
            "band": float(np.float32(band)), "max_planes": int(max_planes), "min_cells": int(min_cells),
            "min_weight": float(np.float32(min_weight)), "iterations": int(iterations)}


# ---- the host steps between the kernels (fp64 NumPy) ------------------------------------------------------------------------
def cube_centres(bins):
    """float64 [6 * bins * bins, 3]: the unit directions of the cube map's bin centres, in gs_tsdf_plane_votes' order (face
    2 m + (g_m < 0), then the bins of the two other axes in increasing order)."""
    t = (np.arange(bins, dtype=np.float64) + 0.5) / (bins // 2) - 1.0
    out = np.zeros((6, bins, bins, 3), np.float64)
    for face in range(6):
        m = face // 2
        b, c = [ax for ax in range(3) if ax != m]
        out[face, :, :, m] = -1.0 if face % 2 else 1.0
        out[face, :, :, b] = t[:, None]
        out[face, :, :, c] = t[None, :]
    out = out.reshape(-1, 3)
    return out / np.linalg.norm(out, axis=1, keepdims=True)


def vote_peaks(votes, cone_deg, max_dirs, min_cells):
    """The peaks of the votes by a cone-weighted mean shift over the bin centres: float64 [P,3] unit directions, P <=
    max_dirs, in the order found.  Seeds are the bins by descending count (ties: the lower index); a bin inside the cone
    of an earlier peak is no seed.  From a seed d, d <- the normalised sum of count * (c . d - cos cone) * c over the
    centres c inside the cone about d, until d stops moving.  A peak counts when the votes inside its cone are at least
    min_cells and it is no earlier peak again."""
    votes = np.asarray(votes)
    bins = votes.shape[-1]
    C = cube_centres(bins)
    w = votes.reshape(-1).astype(np.float64)
    cosc = math.cos(math.radians(cone_deg))
    claimed = np.zeros(w.shape, bool)
    dirs = []
    for seed in np.argsort(-w, kind="stable"):
        if len(dirs) >= max_dirs or w[seed] == 0:
            break
        if claimed[seed]:
            continue
        d = C[seed]
        for _ in range(MEAN_SHIFT_ROUNDS):
            dots = C @ d
            k = np.where(dots >= cosc, w * (dots - cosc), 0.0)
            k[seed] = max(k[seed], w[seed] * 1e-12)             # a cone narrower than a bin still holds its seed
            m = k @ C
            new = m / np.linalg.norm(m)
            moved = float(new @ d)
            d = new
            if moved >= 1.0 - 1e-15:
                break
        inside = C @ d >= cosc
        again = any(float(d @ e) >= cosc for e in dirs)
        claimed |= inside
        claimed[seed] = True
        if not again and w[inside].sum() >= min_cells:
            dirs.append(d)
    return np.array(dirs, np.float64).reshape(-1, 3)


def box_corners(dims, lo, voxel):
    """float64 [8,3]: the corners of the lattice's box."""
    lo = np.asarray(lo, np.float64)
    hi = lo + (np.asarray(dims, np.float64) - 1.0) * float(voxel)
    return np.array([[(lo, hi)[i][0], (lo, hi)[j][1], (lo, hi)[k][2]] for i in (0, 1) for j in (0, 1) for k in (0, 1)])


def box_centre32(dims, lo, voxel):
    """float32 [3]: the middle of the lattice's box, formed in fp64 and rounded once: the moments' reference point."""
    return (np.asarray(lo, np.float64) + 0.5 * (np.asarray(dims, np.float64) - 1.0) * float(voxel)).astype(np.float32)


def offset_bins(dims, lo, voxel, normals, bin_m):
    """How the offsets along `normals` [P,3] are binned: (o0 float64 [P], each representable in fp32; bin, likewise;
    n_bins <= 2048).  Direction j's bin k covers o0[j] + [k, k + 1) bin; o0 lies a bin below the box, and the bin widens
    beyond bin_m when the box's diagonal needs more than 2048 of them."""
    proj = box_corners(dims, lo, voxel) @ np.asarray(normals, np.float64).reshape(-1, 3).T          # [8,P]
    span = float((proj.max(0) - proj.min(0)).max()) if proj.shape[1] else 0.0
    bin_m = float(np.float32(max(float(bin_m), span / (MAX_OFFSET_BINS - 4))))
    n_bins = min(MAX_OFFSET_BINS, int(math.ceil(span / bin_m)) + 4)
    o0 = (proj.min(0) - 2.0 * bin_m).astype(np.float32).astype(np.float64)
    return o0, bin_m, n_bins


def offset_hypotheses(hist, normals, o0, bin_m, min_cells, max_planes):
    """Plane hypotheses from the offset histograms [P,n_bins]: the local maxima of the 3-bin sum s3 (s3[k] > s3[k - 1] and
    s3[k] >= s3[k + 1]) with at least min_cells, each at the count-weighted middle of its three bins.  -> (planes float64
    [Q,4] = (n, o), the direction each came from int64 [Q]), by descending s3 (ties: direction, then bin), Q <= max_planes."""
    h = np.asarray(hist).astype(np.int64)
    P, n = h.shape
    pad = np.zeros((P, n + 2), np.int64)
    pad[:, 1:-1] = h
    s3 = pad[:, :-2] + pad[:, 1:-1] + pad[:, 2:]
    left = np.concatenate([np.full((P, 1), -1, np.int64), s3[:, :-1]], 1)
    right = np.concatenate([s3[:, 1:], np.full((P, 1), -1, np.int64)], 1)
    js, ks = np.nonzero((s3 >= min_cells) & (s3 > left) & (s3 >= right))
    found = sorted((-int(s3[j, k]), int(j), int(k)) for j, k in zip(js, ks))[:max_planes]
    planes, source = [], []
    for neg, j, k in found:
        mid = (pad[j, k] * (k - 0.5) + pad[j, k + 1] * (k + 0.5) + pad[j, k + 2] * (k + 1.5)) / float(-neg)
        planes.append([*normals[j], o0[j] + bin_m * mid])
        source.append(j)
    return np.array(planes, np.float64).reshape(-1, 4), np.array(source, np.int64)


def _covariance(row):
    n = row[10]
    mean = row[:3] / n
    s = row[3:9] / n
    S = np.array([[s[0], s[1], s[2]], [s[1], s[3], s[4]], [s[2], s[4], s[5]]])
    return mean, S - np.outer(mean, mean)


def planes_update(rows, planes, toward, ref):
    """One round of the fit: every plane with at least three inliers becomes the least-squares plane of its inliers, the
    smallest eigenvector of their 3 x 3 covariance (signed to agree with `toward` [P,3], the votes' directions) through
    their centroid.  rows: gs_tsdf_plane_moments' [P,16]; ref: the point the moments were taken about."""
    new = np.array(planes, np.float64)
    for j, row in enumerate(rows):
        if row[10] < 3:
            continue
        mean, cov = _covariance(row)
        v = np.linalg.eigh(cov)[1][:, 0]
        if float(v @ toward[j]) < 0:
            v = -v
        new[j, :3] = v
        new[j, 3] = float(v @ (ref + mean))
    return new


def planes_report(rows, planes, ref, voxel, cone_deg, band, min_cells):
    """The planes' list from their closing rows: count (inliers), rmse_m, centroid, area_m2 = count voxel^2 / (|n0| + |n1|
    + |n2|) (a plane crosses that many cells per voxel^2 of its area); by descending count (ties: the earlier plane);
    planes with fewer than min_cells inliers are dropped, and so is one that lies within cone_deg of a larger one with
    its centroid within `band` of it: two hypotheses that became one plane."""
    cosc = math.cos(math.radians(cone_deg))
    out = []
    for j in sorted(range(len(planes)), key=lambda j: (-rows[j][10], j)):
        count = int(rows[j][10])
        if count < max(min_cells, 1):
            continue
        n, o = planes[j, :3], float(planes[j, 3])
        centroid = ref + rows[j][:3] / count
        if any(float(n @ p["normal"]) >= cosc and abs(float(p["normal"] @ centroid) - p["offset"]) <= band for p in out):
            continue
        out.append({"normal": n.copy(), "offset": o, "count": count, "rmse_m": math.sqrt(rows[j][9] / count),
                    "centroid": centroid, "area_m2": count * voxel * voxel / float(np.abs(n).sum())})
    return out


def find_planes_in(field, args):
    """`find_planes` over a `field` (see the module's text) with `find_arguments`' dict."""
    votes = field.votes(args["bins"], args["min_weight"])
    normals = vote_peaks(votes, args["cone_deg"], args["max_planes"], args["min_cells"])
    if normals.shape[0] == 0:
        return []
    o0, bin_m, n_bins = offset_bins(field.dims, field.lo, field.voxel, normals, args["band"])
    hist = field.offsets(normals, o0, args["cos2"], bin_m, n_bins, args["min_weight"])
    planes, source = offset_hypotheses(hist, normals, o0, bin_m, args["min_cells"], args["max_planes"])
    if planes.shape[0] == 0:
        return []
    toward = normals[source]
    ref32 = box_centre32(field.dims, field.lo, field.voxel)
    ref = ref32.astype(np.float64)
    for _ in range(args["iterations"]):
        rows = field.moments(planes, args["cos2"], args["band"], ref32, args["min_weight"])
        planes = planes_update(rows, planes, toward, ref)
    rows = field.moments(planes, args["cos2"], args["band"], ref32, args["min_weight"])
    return planes_report(rows, planes, ref, float(field.voxel), args["cone_deg"], args["band"], args["min_cells"])


# ---- the kernels over a volume on the GPU -------------------------------------------------------------------------------
class DeviceField:
    """gs_tsdf_plane_* over a TSDFVolume: each method enqueues on the current stream and reads its result once."""

    def __init__(self, vol):
        self.vol, self.dims, self.lo, self.voxel = vol, vol.dims, vol.lo, vol.voxel

    def _lattice(self):
        v = self.vol
        return [_lib.ptr(v.tsdf), _lib.ptr(v.weight), *v.dims]

    def _frame(self):
        v = self.vol
        return [float(v.lo[0]), float(v.lo[1]), float(v.lo[2]), v.voxel]

    def votes(self, bins, min_weight):
        import torch
        dev = self.vol.device
        out = torch.zeros((6, bins, bins), dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            rc = _lib.lib().gs_tsdf_plane_votes(*self._lattice(), min_weight, bins, _lib.ptr(out), _lib.stream_ptr(dev))
        _lib.check(rc, "TSDFVolume.find_planes")
        return out.cpu().numpy().view(np.uint32)

    def offsets(self, normals, o0, cos2, bin_m, n_bins, min_weight):
        import torch
        dev = self.vol.device
        P = int(normals.shape[0])
        n_d = torch.as_tensor(np.ascontiguousarray(normals, np.float64)).to(dev)
        o_d = torch.as_tensor(np.ascontiguousarray(o0, np.float64)).to(dev)
        out = torch.zeros((P, n_bins), dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            rc = _lib.lib().gs_tsdf_plane_offsets(*self._lattice(), *self._frame(), min_weight, _lib.ptr(n_d), _lib.ptr(o_d), P,
                                                  cos2, bin_m, n_bins, _lib.ptr(out), _lib.stream_ptr(dev))
        _lib.check(rc, "TSDFVolume.find_planes")
        return out.cpu().numpy().view(np.uint32)

    def moments(self, planes, cos2, band, ref32, min_weight):
        import torch
        dev = self.vol.device
        P = int(planes.shape[0])
        L = _lib.lib()
        p_d = torch.as_tensor(np.ascontiguousarray(planes, np.float64)).to(dev)
        ws = torch.empty(max(L.gs_tsdf_plane_workspace_bytes(P, *self.vol.dims) // 8, 1), dtype=torch.float64, device=dev)
        out = torch.empty((P, 16), dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            rc = L.gs_tsdf_plane_moments(*self._lattice(), *self._frame(), min_weight, _lib.ptr(p_d), P, cos2, band,
                                         float(ref32[0]), float(ref32[1]), float(ref32[2]), _lib.ptr(ws), _lib.ptr(out),
                                         _lib.stream_ptr(dev))
        _lib.check(rc, "TSDFVolume.find_planes")
        return out.cpu().numpy()


def find_planes(vol, bins=16, cone_deg=10.0, band=None, max_planes=8, min_cells=64, min_weight=1.0, iterations=3):
    """The dominant planes of the volume, by descending inlier count: a list of {"normal": float64 [3] unit, toward free
    space, "offset": o of n . x = o, "count": surface samples within `band` of the plane whose normal direction lies within
    cone_deg of n, "rmse_m": of those samples' distances, "centroid": float64 [3], "area_m2"}.

    A surface sample is a cell seen `min_weight` times at all eight corners, unsaturated, with a sign change, whose centre
    is at most one voxel from the zero set: the point one Newton step from the centre, with the gradient as its normal
    direction.  The samples' directions vote into a cube map of 6 x bins x bins (read once); its peaks are found by a
    cone-weighted mean shift (`vote_peaks`); along every peak direction the agreeing samples' offsets are binned at `band`
    (read once; default: one voxel) and the local maxima of a 3-bin sum with at least min_cells give at most max_planes (<=
    16) hypotheses; `iterations` rounds of gs_tsdf_plane_moments and a least-squares fit move all of them together, a
    closing round counts, and hypotheses that became one plane are merged.  ValueError for bad arguments, before the
    library or the device is reached."""
    what = "TSDFVolume.find_planes"
    _merge._volume(vol, what, "self")
    args = find_arguments(what, vol.voxel, bins, cone_deg, band, max_planes, min_cells, min_weight, iterations)
    return find_planes_in(DeviceField(vol), args)


# ---- the floor and the upright frame -------------------------------------------------------------------------------------
def _plane(plane, what, name="plane"):
    try:
        n = np.asarray(plane["normal"], np.float64).reshape(-1)
        o = float(plane["offset"])
    except (TypeError, KeyError, ValueError, IndexError):
        raise ValueError(f"{what}: {name} must have a \"normal\" of three numbers and an \"offset\"") from None
    if n.shape != (3,) or not np.isfinite(n).all() or not math.isfinite(o) or abs(float(np.linalg.norm(n)) - 1.0) > 1e-6:
        raise ValueError(f"{what}: {name}'s normal must be a finite unit vector and its offset finite")
    return n / np.linalg.norm(n), o / float(np.linalg.norm(n))


def floor_plane(planes, up_hint, max_tilt_deg=35.0, min_share=0.25):
    """The floor among `find_planes`' planes, by a stated policy: of the planes whose normal lies within max_tilt_deg of
    up_hint and whose count is at least min_share of the largest such plane's, the lowest: the one whose centroid (for a
    plane without one: its point nearest the origin) has the smallest coordinate along up_hint.  A table top or a bed is
    large and level too, but it lies above the floor.  None when no plane qualifies.  ValueError for bad arguments."""
    what = "floor_plane"
    up = _vector3(up_hint, what, "up_hint")
    max_tilt_deg, min_share = float(max_tilt_deg), float(min_share)
    if not 0 <= max_tilt_deg < 90:
        raise ValueError(f"{what}: max_tilt_deg must lie in [0, 90) (got {max_tilt_deg})")
    if not 0 <= min_share <= 1:
        raise ValueError(f"{what}: min_share must lie in [0, 1] (got {min_share})")
    cost = math.cos(math.radians(max_tilt_deg))
    level = []
    for i, p in enumerate(planes):
        n, o = _plane(p, what, f"plane {i}")
        if float(n @ up) >= cost:
            at = np.asarray(p["centroid"], np.float64) if p.get("centroid") is not None else o * n
            level.append((float(at @ up), i, int(p.get("count", 0))))
    if not level:
        return None
    largest = max(c for _, _, c in level)
    return planes[min((h, i) for h, i, c in level if c >= min_share * largest)[1]]


def _rotation_onto(n, t):
    """The smallest rotation that takes the unit vector n onto the unit vector t: the turn about a = n x t that carries
    the frame (n, a, n x a) to (t, a, t x a), which is well conditioned at every angle.  Where n x t vanishes (t = n: the
    identity; t = -n: a half turn) a is the direction perpendicular to n that is nearest a coordinate plane."""
    v = np.cross(n, t)
    if float(np.linalg.norm(v)) < 1e-14:
        e = np.zeros(3)
        e[int(np.argmin(np.abs(n)))] = 1.0
        v = np.cross(n, e)
    a = v / np.linalg.norm(v)
    return np.stack([t, a, np.cross(t, a)], 1) @ np.stack([n, a, np.cross(n, a)], 1).T


def upright_transform(plane, up_axis=2, up_sign=+1, wall=None):
    """float64 [4,4], world to map: the smallest rotation that takes the plane's normal onto up_sign e_up_axis, and the
    translation along that axis that puts the plane at coordinate 0.  With `wall`, a plane roughly perpendicular to the
    floor, the smallest further rotation about up (modulo a quarter turn) that lays the wall's horizontal normal along a
    lattice axis.  ValueError for bad arguments."""
    what = "upright_transform"
    n, o = _plane(plane, what)
    if up_axis not in (0, 1, 2) or up_sign not in (1, -1):
        raise ValueError(f"{what}: up_axis must be 0, 1 or 2 and up_sign +1 or -1 (got {up_axis}, {up_sign})")
    t = np.zeros(3)
    t[up_axis] = float(up_sign)
    R = _rotation_onto(n, t)
    if wall is not None:
        w, _ = _plane(wall, what, "wall")
        a, b = (up_axis + 1) % 3, (up_axis + 2) % 3           # a turn by phi about e_up takes e_a toward e_b
        h = R @ w
        if math.hypot(h[a], h[b]) < 0.5:
            raise ValueError(f"{what}: the wall is not roughly perpendicular to the floor")
        phi = math.atan2(h[b], h[a])
        delta = round(phi / (0.5 * math.pi)) * (0.5 * math.pi) - phi
        Z = np.eye(3)
        Z[a, a], Z[a, b], Z[b, a], Z[b, b] = math.cos(delta), -math.sin(delta), math.sin(delta), math.cos(delta)
        R = Z @ R
    U, _, Vt = np.linalg.svd(R)                                 # the nearest rotation: the products above rounded
    R = U @ Vt
    T = np.eye(4)
    T[:3, :3] = R
    T[up_axis, 3] = -float((R @ n)[up_axis]) * o                # (R x)_up = (R n)_up (n . x) on the plane
    _merge.transforms34(T, what)
    return T


def wall_plane(planes, floor, max_deg=WALL_DEG):
    """The largest of `planes` within max_deg of perpendicular to `floor`, or None."""
    n, _ = _plane(floor, "wall_plane", "floor")
    lim = math.sin(math.radians(max_deg))
    walls = [p for p in planes if abs(float(np.asarray(p["normal"], np.float64) @ n)) <= lim]
    return max(walls, key=lambda p: p["count"]) if walls else None


def upright_volume(vol, plane=None, up_hint=None, up_axis=2, up_sign=+1, heading=None, voxel_size=None, planes=None,
                   max_tilt_deg=35.0, min_share=0.25, **find_args):
    """(a new TSDFVolume in the map frame, T float64 [4,4] world to map): the volume resampled (`union_volume` of its moved
    box, then `merge_volume`: gs_tsdf_merge) so that `plane` is the lattice's coordinate 0 along up_axis and its normal
    up_sign e_up_axis.  plane=None: `floor_plane` of `planes` (None: `find_planes(**find_args)`) under up_hint; ValueError
    when that finds no floor.  heading="walls" also turns the map about up so that `wall_plane` faces a lattice axis
    (nothing when there is no wall).  voxel_size: the map's (default: the volume's).  ValueError for bad arguments, before
    the library or the device is reached."""
    what = "TSDFVolume.upright"
    _merge._volume(vol, what, "self")
    if heading not in (None, "walls"):
        raise ValueError(f"{what}: heading must be None or \"walls\" (got {heading!r})")
    if up_axis not in (0, 1, 2) or up_sign not in (1, -1):
        raise ValueError(f"{what}: up_axis must be 0, 1 or 2 and up_sign +1 or -1 (got {up_axis}, {up_sign})")
    if voxel_size is not None and not (float(voxel_size) > 0 and math.isfinite(float(voxel_size))):
        raise ValueError(f"{what}: voxel_size must be positive and finite (got {voxel_size})")
    if plane is None:
        if up_hint is None:
            raise ValueError(f"{what}: without a plane, up_hint must say roughly where up is")
        up_hint = _vector3(up_hint, what, "up_hint")
    else:
        _plane(plane, what)
    if planes is None and (plane is None or heading == "walls"):
        args = find_arguments(what, vol.voxel, **find_args)
        planes = find_planes_in(DeviceField(vol), args)
    if plane is None:
        plane = floor_plane(planes, up_hint, max_tilt_deg, min_share)
        if plane is None:
            raise ValueError(f"{what}: no floor among {len(planes)} planes within {max_tilt_deg} degrees of up_hint "
                             f"{up_hint.tolist()}")
    wall = wall_plane(planes, plane) if heading == "walls" else None
    T = upright_transform(plane, up_axis, up_sign, wall)
    out = _merge.union_volume([vol], [T], voxel_size)
    _merge.merge_volume(out, vol, T)
    return out, T


def moved_poses(T, c2w_list):
    """float32 [N,4,4] (host): the camera-to-world poses c2w_list ([4,4] or [3,4] each) in the frame T [4,4] maps their
    world to; the product is formed in fp64 and rounded once."""
    import torch
    T = torch.as_tensor(np.asarray(T, np.float64))
    out = torch.eye(4, dtype=torch.float64).repeat(len(c2w_list), 1, 1)
    for i, c in enumerate(c2w_list):
        out[i, :3, :] = torch.as_tensor(c).detach().cpu().double()[:3, :]
    return (T @ out).float()


def moved_point(T, point):
    """A world point (three numbers) in the frame T [4,4] maps the world to: a list of three floats."""
    import torch
    p = np.asarray(point.detach().cpu() if isinstance(point, torch.Tensor) else point, np.float64).reshape(-1)
    if p.shape != (3,):
        raise ValueError(f"a world point must be three numbers (got {p.tolist()})")
    T = np.asarray(T, np.float64)
    return (T[:3, :3] @ p + T[:3, 3]).tolist()


_TRANSFORM_HEAD = "Transform from the run's world to the map frame"


def transform_text(T):
    """The text of map/upright.txt: a header line, then the four rows of T with repr() numbers."""
    T = np.asarray(T, np.float64).reshape(4, 4)
    return "\n".join([_TRANSFORM_HEAD + " (the floor is the map's coordinate 0 along its up axis): four rows of a 4 x 4 "
                      "matrix, x_map = R x_world + t"] + [" ".join(repr(float(v)) for v in row) for row in T]) + "\n"


def parse_transform(text):
    """transform_text's inverse: float64 [4,4]."""
    lines = text.splitlines()
    if len(lines) != 5 or not lines[0].startswith(_TRANSFORM_HEAD):
        raise ValueError("not a map/upright.txt")
    T = np.array([[float(v) for v in line.split(" ")] for line in lines[1:]], np.float64)
    if T.shape != (4, 4):
        raise ValueError("map/upright.txt: the transform is not four rows of four numbers")
    return T


# ---- metrics_tsdf_planes.txt ----------------------------------------------------------------------------------------------
_PLANES_HEAD = "Dominant planes of the fused TSDF volume"


def planes_text(planes, floor=None):
    """The text of metrics_tsdf_planes.txt: two header lines, the number of planes, the floor's index (-1: none), then a
    line per plane.  Numbers are written with repr(): `parse_planes` gives them back bit for bit."""
    index = -1
    if floor is not None:
        index = next(i for i, p in enumerate(planes) if p is floor)
    lines = [_PLANES_HEAD + ", by descending inlier count: n . x = offset with the unit normal n toward free space, the "
             "surface samples within the band whose normal direction agrees, the rmse of their distances [m], their "
             "centroid and the area they cover [m^2]",
             "(per plane: count n0 n1 n2 offset rmse_m c0 c1 c2 area_m2; floor is the index of the plane chosen as the "
             "floor, -1 for none)",
             f"planes\t{len(planes)}", f"floor\t{index}"]
    for p in planes:
        vals = [*p["normal"], p["offset"], p["rmse_m"], *p["centroid"], p["area_m2"]]
        lines.append(" ".join([repr(int(p["count"]))] + [repr(float(v)) for v in vals]))
    return "\n".join(lines) + "\n"


def parse_planes(text):
    """planes_text's inverse: (planes, the floor's index or None)."""
    lines = text.splitlines()
    if len(lines) < 4 or not lines[0].startswith(_PLANES_HEAD) or not lines[2].startswith("planes\t") or \
            not lines[3].startswith("floor\t"):
        raise ValueError("not a metrics_tsdf_planes.txt")
    n, floor = int(lines[2].split("\t")[1]), int(lines[3].split("\t")[1])
    if len(lines) != 4 + n or not -1 <= floor < n:
        raise ValueError("metrics_tsdf_planes.txt: the plane count and the lines disagree")
    planes = []
    for line in lines[4:]:
        f = line.split(" ")
        if len(f) != 10:
            raise ValueError("metrics_tsdf_planes.txt: a plane is not ten numbers")
        v = [float(x) for x in f[1:]]
        planes.append({"normal": np.array(v[0:3], np.float64), "offset": v[3], "count": int(f[0]), "rmse_m": v[4],
                       "centroid": np.array(v[5:8], np.float64), "area_m2": v[8]})
    return planes, (None if floor < 0 else floor)
