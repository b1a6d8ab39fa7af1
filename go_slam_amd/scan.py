"""Where on the map is the robot: planar range scans on a 2-D occupancy map and the exhaustive correlative scan match
(csrc/scan.hip; include/goslam_hip.h, gs_scan_*; tests/scan_restatement.py).

A map is the dict of `ESDF.occupancy_slice`, `ESDF.floor_map` or `load_map`: "cells" uint8 [n_u,n_v] with each side in
[1, 1024], "origin", "resolution".  Cell 254 is free, 205 is unknown and every other value is occupied -- the conservative
reading of `plan_on_map`, where only 254 passes.  A pose is a cell (u, v) and a yaw: yaw 0 looks along +u and a positive
yaw turns toward +v, the convention of `view.ray_directions`.  Robot positions are cell centres; a metric pose is origin +
(cell + 0.5) * resolution.  Everything here is exact to the cell and to the yaw step and promises no more than that.

`scan_on_map` is a virtual range scanner (`cast`, gs_scan_cast: one lane per pose and beam, view gain's walk on two
axes).  `cost_field` is the map's likelihood field (`field`, gs_scan_field: the squared distance to the nearest occupied
cell, capped).  `match_scan` scores every (yaw, cell) of a window against a measured scan (`match`, gs_scan_match: the sum
over the beams of the field at the beams' end points) and `localize_on_map` puts the three together and checks the best
pose by casting a scan from it.  The kernels are integer and equal the serial restatement bit for bit; the beam end points
are made on the host in float64 by `beam_offsets`, which the restatement's callers use too.  `scan_localize_text` /
`parse_scan_localize` are a run's map/scan_localize.txt (`scan_config`, `localize_poses`).
"""
import math

import numpy as np
import torch

from . import _lib
from . import plan as _plan

MAX_CELLS = _plan.MAX_CELLS            # per side
MAP_FREE, MAP_OCCUPIED, MAP_UNKNOWN = 254, 0, 205
MAX_DIR = 32767                        # GS_VIEW_MAX_DIR
MAX_BEAMS = 4096
MAX_YAWS = 1024
MAX_RANGE2 = 2 * 1023 * 1023
MAX_LANES = 1 << 28                    # rays of one cast, candidates of one match launch
R_MIN, R_MAX = 1, 15
NO_SCORE = -1                          # the u32 word 0xffffffff read as int32
NO_BEST = 0xffffffffffffffff
KIND_NONE, KIND_HIT, KIND_UNKNOWN = 0, 1, 2


def _int(v, lo, hi, name, what):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
        raise ValueError(f"{what}: {name} must be an integer in [{lo}, {hi}] (got {v!r})")
    return int(v)


def _flag(v, name, what):
    if not isinstance(v, (bool, np.bool_)):
        raise ValueError(f"{what}: {name} must be a bool (got {v!r})")
    return bool(v)


def _number(v, name, what, positive=False):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or math.isnan(float(v)) \
            or float(v) < 0 or (positive and not float(v) > 0):
        raise ValueError(f"{what}: {name} must be a number {'> 0' if positive else '>= 0'} (got {v!r})")
    return float(v)


def _map_tensor(t, name, what, shape=None):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 2 \
            or not all(1 <= int(n) <= MAX_CELLS for n in t.shape) or (shape is not None and tuple(t.shape) != tuple(shape)):
        want = f"[n_u,n_v] with both sizes in [1, {MAX_CELLS}]" if shape is None else str(list(shape))
        raise ValueError(f"{what}: {name} must be a uint8 tensor {want} "
                         f"(got {getattr(t, 'dtype', type(t).__name__)} {list(getattr(t, 'shape', []))})")
    return t


def _on_gpu(t, name, what):
    if not t.is_cuda:
        raise ValueError(f"{what}: {name} must be on a GPU (it is on {t.device}); there is no host path")


def _out(out, specs, dev, what):
    """The output tensors: new ones, or the tuple `out` checked against (name, dtype, shape) of `specs`."""
    if out is None:
        return tuple(torch.empty(shape, dtype=dtype, device=dev) for _, dtype, shape in specs)
    if not isinstance(out, (tuple, list)) or len(out) != len(specs):
        raise ValueError(f"{what}: out must be the {len(specs)} tensors ({', '.join(s[0] for s in specs)})")
    for t, (name, dtype, shape) in zip(out, specs):
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != tuple(shape) or t.device != dev \
                or not t.is_contiguous():
            raise ValueError(f"{what}: out {name} must be a contiguous {str(dtype).replace('torch.', '')} tensor "
                             f"{list(shape)} on {dev}")
    return tuple(out)


def _rows(a, name, dtype_name, cols, what, dev):
    """`a` (a tensor or an array of integers whose last size is `cols`) as a contiguous int32 tensor on `dev`."""
    if isinstance(a, torch.Tensor):
        if a.is_floating_point() or a.dtype == torch.bool or a.dim() < 2 or a.shape[-1] != cols:
            raise ValueError(f"{what}: {name} must be integers {dtype_name} (got {a.dtype} {list(a.shape)})")
        if a.dtype != torch.int32:
            if a.numel() and not -0x80000000 <= int(a.min()) <= int(a.max()) <= 0x7fffffff:
                raise ValueError(f"{what}: a value of {name} does not fit 32 bits")
            a = a.to(torch.int32)
        return a.to(dev).contiguous()
    arr = np.asarray(a)
    if arr.ndim < 2 or arr.shape[-1] != cols or not (np.issubdtype(arr.dtype, np.integer) and arr.dtype != np.bool_):
        raise ValueError(f"{what}: {name} must be integers {dtype_name} (got {arr.dtype} {list(arr.shape)})")
    if arr.size and not -0x80000000 <= int(arr.min()) <= int(arr.max()) <= 0x7fffffff:
        raise ValueError(f"{what}: a value of {name} does not fit 32 bits")
    return torch.from_numpy(np.array(arr, dtype=np.int32, order="C")).to(dev)    # a copy: the array may be read-only


# ---- the three kernels --------------------------------------------------------------------------------------------------
@torch.no_grad()
def cast(cells, poses, dirs, range2, stop_unknown=True, out=None):
    """gs_scan_cast over the map cells uint8 [n_u,n_v]: poses integers [P,2] (cells), dirs integers [P,B,2] with every
    component in [-32767, 32767], range2 the squared range in cells.  -> (kind uint8 [P,B]: 0 no return, 1 hit, 2 stopped
    at an unknown cell; hit int32 [P,B], the linear index u * n_v + v of the cell that ended the ray, or -1; range_mc int32
    [P,B], floor(1000 * sqrt(du^2 + dv^2)) of that cell's offset, or -1) on the map's device; `out` = (kind, hit, range_mc)
    writes into given tensors.  A pose outside the map, a zero direction and a direction out of range cast nothing.
    Enqueues on the current stream and reads nothing back.  ValueError before the device is touched."""
    what = "scan.cast"
    _map_tensor(cells, "cells", what)
    range2 = _int(range2, 1, MAX_RANGE2, "range2", what)
    stop_unknown = _flag(stop_unknown, "stop_unknown", what)
    _on_gpu(cells, "cells", what)
    dev = cells.device
    poses = _rows(poses, "poses", "[P,2]", 2, what, dev)
    dirs = _rows(dirs, "dirs", "[P,B,2]", 2, what, dev)
    if poses.dim() != 2 or dirs.dim() != 3 or dirs.shape[0] != poses.shape[0]:
        raise ValueError(f"{what}: poses must be [P,2] and dirs [P,B,2] (got {list(poses.shape)}, {list(dirs.shape)})")
    P, B = int(poses.shape[0]), int(dirs.shape[1])
    if not 1 <= B <= MAX_BEAMS or P * B > MAX_LANES:
        raise ValueError(f"{what}: {P} poses of {B} beams; 1 to {MAX_BEAMS} beams and at most 2^28 rays are allowed")
    kind, hit, range_mc = _out(out, (("kind", torch.uint8, (P, B)), ("hit", torch.int32, (P, B)),
                                     ("range_mc", torch.int32, (P, B))), dev, what)
    cells = cells.contiguous()
    n_u, n_v = (int(n) for n in cells.shape)
    with torch.cuda.device(dev):
        rc = _lib.lib().gs_scan_cast(_lib.ptr(cells), n_u, n_v, _lib.ptr(poses), P, _lib.ptr(dirs), B, range2,
                                     int(stop_unknown), _lib.ptr(kind), _lib.ptr(hit), _lib.ptr(range_mc),
                                     _lib.stream_ptr(dev))
    _lib.check(rc, what)
    return kind, hit, range_mc


@torch.no_grad()
def field(cells, radius_cells=6, out=None):
    """gs_scan_field: uint8 [n_u,n_v] on the map's device, min(d2, R * R + 1) with d2 the exact squared distance in cells
    to the nearest occupied cell (unknown cells are no sites) and R = radius_cells in [1, 15]; `out` = (cost,) writes into
    a given tensor.  Enqueues on the current stream and reads nothing back.  ValueError before the device is touched."""
    what = "scan.field"
    _map_tensor(cells, "cells", what)
    R = _int(radius_cells, R_MIN, R_MAX, "radius_cells", what)
    _on_gpu(cells, "cells", what)
    dev = cells.device
    shape = tuple(int(n) for n in cells.shape)
    cost, = _out(out, (("cost", torch.uint8, shape),), dev, what)
    cells = cells.contiguous()
    with torch.cuda.device(dev):
        rc = _lib.lib().gs_scan_field(_lib.ptr(cells), shape[0], shape[1], R, _lib.ptr(cost), _lib.stream_ptr(dev))
    _lib.check(rc, what)
    return cost


def _window(window, shape, what):
    """(u0, v0, w_u, w_v) inside a map of `shape`; None is the whole map."""
    if window is None:
        return 0, 0, int(shape[0]), int(shape[1])
    try:
        u0, v0, w_u, w_v = window
    except (TypeError, ValueError):
        raise ValueError(f"{what}: window must be (u0, v0, w_u, w_v) in cells or None (got {window!r})") from None
    u0, v0 = _int(u0, 0, shape[0] - 1, "window u0", what), _int(v0, 0, shape[1] - 1, "window v0", what)
    return u0, v0, _int(w_u, 1, shape[0] - u0, "window w_u", what), _int(w_v, 1, shape[1] - v0, "window w_v", what)


@torch.no_grad()
def match(cost, cells, offsets, window=None, cap=None, allow_unknown=False, out=None):
    """gs_scan_match: cost (of `field`) and cells uint8 [n_u,n_v], offsets integers [Y,B,2] (per yaw hypothesis the cell
    offset of every beam's end point from the robot's cell), window (u0, v0, w_u, w_v) in cells (None: the whole map) with
    Y * w_u * w_v <= 2^28, cap the cost of an end point outside the map.  -> (score int32 [Y,w_u,w_v], the kernel's u32 words: -1 (0xffffffff)
    where the robot's cell is not free -- with `allow_unknown` an unknown cell counts as free --, else the sum of the field
    at the end points; best int64 [1], the kernel's u64 word: the smallest (score << 32) | linear index over the candidates
    that may stand, -1 (all ones) without one) on the map's device; `out` = (score, best) writes into given tensors.  Ties go to the lowest index
    and every run gives the same bits.  Enqueues on the current stream and reads nothing back.  ValueError before the
    device is touched."""
    what = "scan.match"
    _map_tensor(cost, "cost", what)
    _map_tensor(cells, "cells", what, tuple(cost.shape))
    n_u, n_v = (int(n) for n in cost.shape)
    u0, v0, w_u, w_v = _window(window, (n_u, n_v), what)
    cap = _int(cap, 1, R_MAX * R_MAX + 1, "cap", what)
    allow_unknown = _flag(allow_unknown, "allow_unknown", what)
    _on_gpu(cost, "cost", what)
    dev = cost.device
    if cells.device != dev:
        raise ValueError(f"{what}: cells must be on {dev} like cost (it is on {cells.device})")
    offsets = _rows(offsets, "offsets", "[Y,B,2]", 2, what, dev)
    if offsets.dim() != 3:
        raise ValueError(f"{what}: offsets must be [Y,B,2] (got {list(offsets.shape)})")
    Y, B = int(offsets.shape[0]), int(offsets.shape[1])
    if not (1 <= Y <= MAX_YAWS and 1 <= B <= MAX_BEAMS):
        raise ValueError(f"{what}: {Y} yaws of {B} beams; 1 to {MAX_YAWS} yaws and 1 to {MAX_BEAMS} beams are allowed")
    if Y * w_u * w_v > MAX_LANES:
        raise ValueError(f"{what}: {Y} x {w_u} x {w_v} candidates, at most 2^28 in one call")
    score, best = _out(out, (("score", torch.int32, (Y, w_u, w_v)), ("best", torch.int64, (1,))), dev, what)
    cost, cells = cost.contiguous(), cells.contiguous()
    with torch.cuda.device(dev):
        rc = _lib.lib().gs_scan_match(_lib.ptr(cost), _lib.ptr(cells), n_u, n_v, _lib.ptr(offsets), Y, B, u0, v0, w_u,
                                      w_v, cap, int(allow_unknown), _lib.ptr(score), _lib.ptr(best), _lib.stream_ptr(dev))
    _lib.check(rc, what)
    return score, best


# ---- beams on the host (float64) ---------------------------------------------------------------------------------------
def beam_angles(n_beams, fov_deg=360.0):
    """float64 [n_beams] (numpy): the beams' angles from the scanner's forward axis in radians, increasing toward +v, as a
    laser scan message counts them: -fov / 2 + i * increment.  Over the full circle (fov_deg 360) the increment is fov /
    n_beams, so that no direction is taken twice; over less it is fov / (n_beams - 1) and both ends are beams (one beam
    looks forward).  0 < fov_deg <= 360."""
    what = "beam_angles"
    n = _int(n_beams, 1, MAX_BEAMS, "n_beams", what)
    if isinstance(fov_deg, bool) or not isinstance(fov_deg, (int, float, np.integer, np.floating)) \
            or not 0 < float(fov_deg) <= 360:
        raise ValueError(f"{what}: fov_deg must lie in (0, 360] degrees (got {fov_deg!r})")
    fov = math.radians(float(fov_deg))
    if n == 1:
        return np.zeros(1, dtype=np.float64)
    return np.arange(n, dtype=np.float64) * (fov / (n if float(fov_deg) == 360.0 else n - 1)) - 0.5 * fov


def _angles(angles, what):
    a = np.asarray(angles.detach().cpu().numpy() if isinstance(angles, torch.Tensor) else angles, dtype=np.float64)
    if a.ndim != 1 or not 1 <= a.shape[0] <= MAX_BEAMS or not np.isfinite(a).all():
        raise ValueError(f"{what}: angles must be 1 to {MAX_BEAMS} finite numbers [B] (got {list(a.shape)})")
    return a


def _yaws(yaws, what, name="yaws"):
    y = np.asarray(yaws.detach().cpu().numpy() if isinstance(yaws, torch.Tensor) else yaws, dtype=np.float64)
    if y.ndim > 1 or not np.isfinite(y).all():
        raise ValueError(f"{what}: {name} must be a finite number or finite numbers [Y] (got shape {list(y.shape)})")
    return y


def beam_directions(angles, yaw):
    """int32 [B,2] for a number `yaw`, [P,B,2] for yaws [P] (numpy): the direction (cos, sin)(angle + yaw) of every beam
    along (u, v), scaled so that its largest component is GS_VIEW_MAX_DIR and rounded to nearest.  Host float64, as in
    `view.ray_directions`."""
    what = "beam_directions"
    a = _angles(angles, what)
    y = _yaws(yaw, what, "yaw")
    t = y[..., None] + a
    d = np.stack([np.cos(t), np.sin(t)], axis=-1)
    d *= MAX_DIR / np.abs(d).max(axis=-1, keepdims=True)
    return np.rint(d).astype(np.int32)


def _ranges(ranges_m, n, what):
    r = ranges_m.detach().cpu().numpy() if isinstance(ranges_m, torch.Tensor) else np.asarray(ranges_m)
    if r.ndim != 1 or r.shape[0] != n or not (np.issubdtype(r.dtype, np.floating) or np.issubdtype(r.dtype, np.integer)):
        raise ValueError(f"{what}: ranges_m must be numbers [{n}], one per angle (got {r.dtype} {list(r.shape)})")
    return r.astype(np.float64)


def _range_limits(min_range, max_range, what):
    lo = _number(min_range, "min_range", what)
    hi = _number(max_range, "max_range", what, positive=True)
    if lo > hi:
        raise ValueError(f"{what}: min_range {lo} lies above max_range {hi}")
    return lo, hi


def valid_beams(ranges_m, min_range=0.0, max_range=math.inf):
    """bool [B] (numpy): the beams `beam_offsets` keeps, finite with min_range <= r <= max_range."""
    r = np.asarray(ranges_m.detach().cpu().numpy() if isinstance(ranges_m, torch.Tensor) else ranges_m, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.isfinite(r) & (r >= min_range) & (r <= max_range)


def beam_offsets(ranges_m, angles, yaws, resolution, min_range=0.0, max_range=math.inf):
    """int32 [Y,B',2] (numpy): per yaw hypothesis the cell offset of every valid beam's end point from the robot's cell,
    du = floor(r * cos(angle + yaw) / resolution + 0.5) and dv likewise with sin, in numpy float64.  The beams that are not
    finite or lie outside [min_range, max_range] are dropped once, not per yaw (`valid_beams`); B' may be 0.  An offset
    beyond the 32 bits of the result is clamped there (the match counts anything beyond 16 bits as outside the map)."""
    what = "beam_offsets"
    a = _angles(angles, what)
    r = _ranges(ranges_m, a.shape[0], what)
    y = np.atleast_1d(_yaws(yaws, what))
    res = _number(resolution, "resolution", what, positive=True)
    lo, hi = _range_limits(min_range, max_range, what)
    keep = valid_beams(r, lo, hi)
    r, a = r[keep], a[keep]
    t = y[:, None] + a[None, :]
    off = np.stack([np.floor(r[None, :] * np.cos(t) / res + 0.5), np.floor(r[None, :] * np.sin(t) / res + 0.5)], axis=-1)
    return np.clip(off, -0x7fffffff, 0x7fffffff).astype(np.int32)


# ---- on a map dict ------------------------------------------------------------------------------------------------------
def _grid(grid, what, device=None):
    """(cells as given, origin, resolution, device) of a map dict, or ValueError.  Touches no device."""
    if not isinstance(grid, dict) or any(k not in grid for k in ("cells", "origin", "resolution")):
        raise ValueError(f"{what}: grid must be a map dict with cells, origin and resolution")
    cells = grid["cells"]
    if not isinstance(cells, torch.Tensor):
        cells = np.asarray(cells)
        if cells.dtype.kind not in "uib":
            raise ValueError(f"{what}: cells must be uint8 [n_u,n_v] (got {cells.dtype})")
        cells = torch.from_numpy(np.array(cells, order="C"))           # a copy: the caller's array may be read-only
    if cells.dim() != 2 or cells.dtype != torch.uint8 or not all(1 <= int(n) <= MAX_CELLS for n in cells.shape):
        raise ValueError(f"{what}: cells must be uint8 [n_u,n_v] with both sizes in [1, {MAX_CELLS}] "
                         f"(got {cells.dtype} {list(cells.shape)})")
    res = float(grid["resolution"])
    try:
        origin = [float(v) for v in grid["origin"]][:2]
    except (TypeError, ValueError):
        raise ValueError(f"{what}: origin must be (x, y) (got {grid['origin']!r})") from None
    if not (res > 0 and math.isfinite(res)) or len(origin) != 2 or not all(math.isfinite(v) for v in origin):
        raise ValueError(f"{what}: resolution must be positive and the origin finite (got {res}, {origin})")
    if device is None:
        device = cells.device if cells.is_cuda else torch.device("cuda")
    return cells, origin, res, torch.device(device)


def _range2(range_m, res, shape, what):
    """The squared range in cells of gs_scan_cast for a range in metres; None reaches across the whole map."""
    if range_m is None:
        return min(int(shape[0]) ** 2 + int(shape[1]) ** 2, MAX_RANGE2)
    r = _number(range_m, "max_range", what, positive=True) / res
    return int(min(max(math.floor(r * r), 1.0), float(MAX_RANGE2)))


@torch.no_grad()
def scan_on_map(grid, pose_xy, yaw, n_beams=360, fov_deg=360.0, max_range=None, stop_unknown=True, device=None):
    """The range scan a planar scanner at `pose_xy` (map coordinates, metres) looking along `yaw` (radians) would measure
    on the map `grid`: n_beams beams over fov_deg degrees (`beam_angles`), each walked cell by cell from the centre of the
    pose's cell floor((xy - origin) / resolution) to the first occupied cell within `max_range` metres (None: the whole
    map); with `stop_unknown` an unknown cell ends a beam without a return.  pose_xy (x, y) with a number yaw gives [B]
    results, pose_xy [P,2] with yaws [P] gives [P,B].  -> {"angles": float64 [B] (numpy), "ranges_m": float64, the
    distance between the centres of the pose's cell and the hit cell rounded down to a thousandth of a cell, NaN without a
    return, "kind": uint8 (0 no return, 1 hit, 2 stopped at unknown), "hit": int32 linear cell index or -1, "cells": int32
    the poses' cells}, tensors on the map's device (a host map goes to `device`, by default the current GPU).  Exact to
    the cell: the scanner stands at the cell's centre.  ValueError for a pose outside the map or a bad argument, before
    the device is touched."""
    what = "scan_on_map"
    cells, origin, res, dev = _grid(grid, what, device)
    angles = beam_angles(n_beams, fov_deg)
    stop_unknown = _flag(stop_unknown, "stop_unknown", what)
    range2 = _range2(max_range, res, cells.shape, what)
    xy = np.asarray(pose_xy.detach().cpu().numpy() if isinstance(pose_xy, torch.Tensor) else pose_xy, dtype=np.float64)
    single = xy.ndim == 1
    y = _yaws(yaw, what, "yaw")
    if xy.ndim not in (1, 2) or xy.shape[-1] != 2 or (single and y.ndim != 0) or (not single and y.shape != xy.shape[:1]):
        raise ValueError(f"{what}: pose_xy must be (x, y) with a number yaw, or [P,2] with yaws [P] "
                         f"(got {list(xy.shape)}, {list(y.shape)})")
    xy, y = xy.reshape(-1, 2), y.reshape(-1)
    poses = np.array([_plan.map_cell(cells.shape, origin, res, p, f"pose {i}", what) for i, p in enumerate(xy)],
                     dtype=np.int32).reshape(-1, 2)
    dirs = beam_directions(angles, y)
    cells = cells.to(dev)
    kind, hit, range_mc = cast(cells, poses, dirs, range2, stop_unknown)
    # a tensor divisor: the division by a number is a multiplication by its rounded inverse on the device
    ranges = range_mc.double() / torch.full_like(range_mc, 1000.0, dtype=torch.float64) * res
    ranges = torch.where(kind == KIND_HIT, ranges, torch.full_like(ranges, math.nan))
    poses = torch.from_numpy(poses).to(dev)
    if single:
        kind, hit, ranges, poses = kind[0], hit[0], ranges[0], poses[0]
    return {"angles": angles, "ranges_m": ranges, "kind": kind, "hit": hit, "cells": poses}


@torch.no_grad()
def cost_field(grid, radius_cells=6, device=None):
    """The likelihood field of the map `grid` (`field`): uint8 [n_u,n_v] on the map's device (a host map goes to `device`,
    by default the current GPU), min(d2, radius_cells^2 + 1) with d2 the squared distance in cells to the nearest
    occupied cell."""
    what = "cost_field"
    cells, _, _, dev = _grid(grid, what, device)
    R = _int(radius_cells, R_MIN, R_MAX, "radius_cells", what)
    return field(cells.to(dev), R)


def _match_arguments(grid, ranges_m, angles, yaws, window, radius_cells, allow_unknown, min_range, max_range, device, what):
    cells, origin, res, dev = _grid(grid, what, device)
    offsets = beam_offsets(ranges_m, angles, yaws, res, min_range, max_range)
    if not 1 <= offsets.shape[0] <= MAX_YAWS:
        raise ValueError(f"{what}: {offsets.shape[0]} yaw hypotheses, 1 to {MAX_YAWS} are allowed")
    window = _window(window, cells.shape, what)
    R = _int(radius_cells, R_MIN, R_MAX, "radius_cells", what)
    return cells, origin, res, dev, offsets, window, R, _flag(allow_unknown, "allow_unknown", what)


@torch.no_grad()
def _match_all(cells, offsets, window, R, allow_unknown):
    """(score int32 [Y,w_u,w_v], best (yaw index, (u, v)) or None, its score or None): `match` over all the yaws, in as
    many launches as keep each below 2^28 candidates, then one read of the launches' best words."""
    Y = int(offsets.shape[0])
    u0, v0, w_u, w_v = window
    cost = field(cells, R)
    step = max(1, min(Y, MAX_LANES // (w_u * w_v)))
    score = torch.empty((Y, w_u, w_v), dtype=torch.int32, device=cells.device)
    starts = list(range(0, Y, step))
    best = torch.empty((len(starts),), dtype=torch.int64, device=cells.device)
    off = torch.from_numpy(offsets).to(cells.device)
    for n, y0 in enumerate(starts):
        match(cost, cells, off[y0:y0 + step], window, R * R + 1, allow_unknown, out=(score[y0:y0 + step], best[n:n + 1]))
    words = best.cpu().tolist()                       # the one read
    found = None
    for y0, word in zip(starts, words):
        word &= NO_BEST
        if word == NO_BEST:
            continue
        s, index = word >> 32, word & 0xffffffff
        y, rest = divmod(index, w_u * w_v)
        key = (s, y0 + y, rest)
        found = key if found is None or key < found else found
    if found is None:
        return score, None, None
    i, j = divmod(found[2], w_v)
    return score, (found[1], (u0 + i, v0 + j)), found[0]


@torch.no_grad()
def match_scan(grid, ranges_m, angles, yaws, window=None, radius_cells=6, allow_unknown=False, min_range=0.0,
               max_range=math.inf, device=None):
    """Score every pose (yaw of `yaws`, cell of `window`) of the map `grid` against the scan (ranges_m [B] in metres at
    `angles` [B] radians): the sum over the valid beams (`beam_offsets`) of the map's `cost_field` of radius_cells at the
    beam's end point, an end point outside the map costing radius_cells^2 + 1.  A pose may stand only on a free cell, with
    `allow_unknown` also on an unknown one.  window (u0, v0, w_u, w_v) in cells, None the whole map.  -> {"score": int32
    [Y,w_u,w_v] on the device (-1 where the robot cannot stand), "best": (yaw index, (u, v)) of the smallest score
    -- ties to the lowest yaw index, then u, then v -- or None when no pose may stand, "best_score", "window", "n_beams":
    the valid beams}.  Exact to the cell and to the spacing of `yaws`.  One small read.  ValueError for a bad argument or a
    scan without a valid beam, before the device is touched."""
    what = "match_scan"
    cells, _, _, dev, offsets, window, R, allow_unknown = _match_arguments(
        grid, ranges_m, angles, yaws, window, radius_cells, allow_unknown, min_range, max_range, device, what)
    if offsets.shape[1] == 0:
        raise ValueError(f"{what}: the scan has no valid beam (finite, within [{min_range}, {max_range}] m)")
    score, best, best_score = _match_all(cells.to(dev), offsets, window, R, allow_unknown)
    return {"score": score, "best": best, "best_score": best_score, "window": window, "n_beams": int(offsets.shape[1])}


def _around(around, n_yaw, shape, origin, res, what):
    """(window, yaw indices) of `localize_on_map`'s `around` = (xy, radius_m, yaw, yaw_radius); None: everything."""
    every = np.arange(n_yaw)
    if around is None:
        return None, every
    try:
        xy, radius_m, yaw, yaw_radius = around
    except (TypeError, ValueError):
        raise ValueError(f"{what}: around must be (xy, radius_m, yaw, yaw_radius) or None (got {around!r})") from None
    window = None
    if xy is not None:
        u, v = _plan.map_cell(shape, origin, res, xy, "around xy", what)
        r = int(min(math.ceil(_number(radius_m, "around radius_m", what) / res), MAX_CELLS))
        u0, v0 = max(u - r, 0), max(v - r, 0)
        window = (u0, v0, min(u + r, shape[0] - 1) - u0 + 1, min(v + r, shape[1] - 1) - v0 + 1)
    if yaw is not None:
        yaw = float(_yaws(yaw, what, "around yaw").reshape(()))
        width = _number(yaw_radius, "around yaw_radius", what)
        step = 2.0 * math.pi / n_yaw
        apart = np.abs((every * step - yaw + math.pi) % (2.0 * math.pi) - math.pi)
        every = every[apart <= width + 1e-12]
        if every.size == 0:                                             # narrower than a step: the nearest hypothesis
            every = np.array([int(round(yaw / step)) % n_yaw])
    return window, every


def reach2(ranges_cells, tol_cells):
    """The squared range in cells of the cast that checks a pose: one cell beyond the longest measured range plus the
    tolerance, so that every return that could be an inlier is seen."""
    reach = min(float(np.max(ranges_cells)) + float(tol_cells) + 1.0, 2048.0)
    return int(min(max(math.floor(reach * reach), 1.0), float(MAX_RANGE2)))


def count_inliers(kind, range_mc, ranges_cells, tol_cells):
    """How many beams of a cast (kind, range_mc [B], numpy) returned within tol_cells of the measured ranges (in cells)."""
    kind, range_mc = np.asarray(kind), np.asarray(range_mc, dtype=np.float64)
    return int(((kind == KIND_HIT) & (np.abs(range_mc / 1000.0 - np.asarray(ranges_cells, dtype=np.float64)) <= tol_cells)).sum())


@torch.no_grad()
def localize_on_map(grid, ranges_m, angles, n_yaw=360, around=None, radius_cells=6, allow_unknown=False, min_range=0.0,
                    max_range=math.inf, tol_cells=2, stop_unknown=True, device=None):
    """Where on the map `grid` was the scan (ranges_m [B] metres at `angles` [B] radians) taken: the exhaustive search of
    `match_scan` over the yaws 2 pi k / n_yaw, k = 0 .. n_yaw - 1, and the cells of the map -- with around = (xy, radius_m,
    yaw, yaw_radius) only the cells within radius_m metres of xy along each axis and the yaws within yaw_radius of yaw (xy
    or yaw None: no limit on that part) --, then one scan cast from the best pose (`cast`, the valid beams only, with
    `stop_unknown`) to count the beams whose cast range lies within tol_cells cells of the measured one.  ->
    {"found", "cell": (u, v), "xy": the cell's centre origin + (cell + 0.5) * resolution, "yaw": 2 pi yaw_index / n_yaw,
    "yaw_index", "score", "mean_cost": score / n_beams, "inliers", "inlier_fraction": inliers / n_beams, "n_beams": the
    valid beams}.  The score does not penalise a beam that crosses a wall; inlier_fraction reports it.  The result is exact
    to the cell and to the yaw step 2 pi / n_yaw, no finer.  A scan with no valid beam, or a search in which no pose may
    stand, gives found False (the first without a launch).  ValueError for a bad argument, before the device is touched."""
    what = "localize_on_map"
    n_yaw = _int(n_yaw, 1, MAX_YAWS, "n_yaw", what)
    tol = _number(tol_cells, "tol_cells", what)
    stop_unknown = _flag(stop_unknown, "stop_unknown", what)
    cells, origin, res, dev = _grid(grid, what, device)
    window, ks = _around(around, n_yaw, cells.shape, origin, res, what)
    yaws = ks * (2.0 * math.pi / n_yaw)
    cells, origin, res, dev, offsets, window, R, allow_unknown = _match_arguments(
        grid, ranges_m, angles, yaws, window, radius_cells, allow_unknown, min_range, max_range, device, what)
    n_beams = int(offsets.shape[1])
    none = {"found": False, "cell": None, "xy": None, "yaw": None, "yaw_index": None, "score": None, "mean_cost": None,
            "inliers": 0, "inlier_fraction": 0.0, "n_beams": n_beams}
    if n_beams == 0:
        return none
    cells = cells.to(dev)
    _, best, best_score = _match_all(cells, offsets, window, R, allow_unknown)
    if best is None:
        return none
    k = int(ks[best[0]])
    cell = best[1]
    a = _angles(angles, what)
    r = _ranges(ranges_m, a.shape[0], what)
    keep = valid_beams(r, min_range, max_range)
    r_cells = r[keep] / res
    kind, _, range_mc = cast(cells, np.array([cell], dtype=np.int32), beam_directions(a[keep], yaws[best[0]])[None],
                             reach2(r_cells, tol), stop_unknown)
    both = torch.stack([kind[0].to(torch.int32), range_mc[0]]).cpu().numpy()       # the one read
    inliers = count_inliers(both[0], both[1], r_cells, tol)
    return {"found": True, "cell": cell, "xy": (origin[0] + (cell[0] + 0.5) * res, origin[1] + (cell[1] + 0.5) * res),
            "yaw": float(k * (2.0 * math.pi / n_yaw)), "yaw_index": k, "score": int(best_score),
            "mean_cost": best_score / n_beams, "inliers": inliers, "inlier_fraction": inliers / n_beams, "n_beams": n_beams}


# ---- a run's map/scan_localize.txt --------------------------------------------------------------------------------------
SCAN_ROW_ORDER = ("true_u", "true_v", "true_yaw", "true_yaw_index", "found_u", "found_v", "found_yaw_index", "score",
                  "inlier_fraction")
_SCAN_ROW_FLOATS = ("true_yaw", "inlier_fraction")
SCAN_SUMMARY_ORDER = ("n_yaw", "poses_tried", "poses_skipped", "poses_recovered")
_SCAN_HEAD = "Scan localisation on the occupancy map"


def scan_config(value, what="fuse_from_config: tsdf.esdf.scan"):
    """None when the config value is absent (or has enable false), else the checked {"up_axis", "height", "beams",
    "fov_deg", "max_range", "every", "n_yaw", "window_m"}: up_axis and height (h0, h1) as in tsdf.esdf.slice, beams and
    fov_deg of `beam_angles`, max_range in metres (None: the whole map), every >= 1, n_yaw in [1, 1024], window_m >= 0
    the half width of the search window in metres.  ValueError for an unknown key or a bad value.  Touches no device."""
    if value is None:
        return None
    keys = {"enable", "up_axis", "height", "beams", "fov_deg", "max_range", "every", "n_yaw", "window_m"}
    if not isinstance(value, dict) or set(value) - keys:
        raise ValueError(f"{what} must be a dict with keys among {sorted(keys)} (got {value!r})")
    if not isinstance(value.get("enable", True), bool):
        raise ValueError(f"{what}.enable must be a bool (got {value['enable']!r})")
    if not value.get("enable", True):
        return None
    missing = sorted(k for k in ("up_axis", "height") if k not in value)
    if missing:
        raise ValueError(f"{what}: missing {missing}")
    up_axis = _int(value["up_axis"], 0, 2, "up_axis", what)
    try:
        h0, h1 = (float(h) for h in value["height"])
    except (TypeError, ValueError):
        raise ValueError(f"{what}.height must be (h0, h1) in metres (got {value['height']!r})") from None
    if math.isnan(h0) or math.isnan(h1) or h0 > h1:
        raise ValueError(f"{what}.height must be (h0, h1) with h0 <= h1 (got {value['height']!r})")
    beams = _int(value.get("beams", 360), 1, MAX_BEAMS, "beams", what)
    fov = value.get("fov_deg", 360.0)
    if isinstance(fov, bool) or not isinstance(fov, (int, float)) or not 0 < float(fov) <= 360:
        raise ValueError(f"{what}.fov_deg must lie in (0, 360] degrees (got {fov!r})")
    max_range = value.get("max_range")
    if max_range is not None:
        max_range = _number(max_range, "max_range", what, positive=True)
    return {"up_axis": up_axis, "height": (h0, h1), "beams": beams, "fov_deg": float(fov),
            "max_range": max_range, "every": _int(value.get("every", 5), 1, 1 << 30, "every", what),
            "n_yaw": _int(value.get("n_yaw", 360), 1, MAX_YAWS, "n_yaw", what),
            "window_m": _number(value.get("window_m", 1.0), "window_m", what)}


def planar_poses(c2w_list, axes):
    """[(xy, yaw) or None] per camera-to-world pose: the camera centre along the map's two `axes` and the yaw of the
    optical axis (the pose's third column) projected onto them; None for a camera that looks along the up axis."""
    out = []
    u, v = (int(a) for a in axes)
    for c2w in c2w_list:
        m = torch.as_tensor(c2w).double().cpu().numpy()
        z = (float(m[u, 2]), float(m[v, 2]))
        out.append(None if math.hypot(*z) < 1e-9 else ((float(m[u, 3]), float(m[v, 3])), math.atan2(z[1], z[0])))
    return out


@torch.no_grad()
def localize_poses(grid, poses, cfg):
    """The dict `scan_localize_text` writes: for every cfg["every"]-th pose of `poses` (`planar_poses`) whose cell on the
    map `grid` is free, a scan cast there (`scan_on_map` with cfg's beams, fov_deg and max_range) and localised within
    cfg["window_m"] of the pose over all cfg["n_yaw"] yaws (`localize_on_map`).  "rows": per pose tried the true cell, yaw
    and nearest yaw index, the found cell and yaw index (-1 when nothing was found), the score and the inlier fraction;
    "poses_skipped": poses outside the map, on a cell that is not free or without a yaw; "poses_recovered": poses found
    again within one cell and one yaw step."""
    what = "scan.localize_poses"
    cells, origin, res, dev = _grid(grid, what)
    host = cells.cpu().numpy()
    n_yaw = cfg["n_yaw"]
    step = 2.0 * math.pi / n_yaw
    rows, skipped, recovered = [], 0, 0
    for pose in poses[::cfg["every"]]:
        cell = None
        if pose is not None:
            try:
                cell = _plan.map_cell(cells.shape, origin, res, pose[0], "pose", what)
            except ValueError:
                cell = None
        if cell is None or host[cell] != MAP_FREE:
            skipped += 1
            continue
        xy, yaw = pose
        scan = scan_on_map(grid, xy, yaw, cfg["beams"], cfg["fov_deg"], cfg["max_range"], True)
        res_l = localize_on_map(grid, scan["ranges_m"], scan["angles"], n_yaw, around=(xy, cfg["window_m"], None, None))
        k_true = int(round(yaw / step)) % n_yaw
        row = {"true_u": cell[0], "true_v": cell[1], "true_yaw": float(yaw), "true_yaw_index": k_true, "found_u": -1,
               "found_v": -1, "found_yaw_index": -1, "score": -1, "inlier_fraction": 0.0}
        if res_l["found"]:
            row.update(found_u=res_l["cell"][0], found_v=res_l["cell"][1], found_yaw_index=res_l["yaw_index"],
                       score=res_l["score"], inlier_fraction=res_l["inlier_fraction"])
            turn = abs(res_l["yaw_index"] - k_true)
            if max(abs(row["found_u"] - cell[0]), abs(row["found_v"] - cell[1])) <= 1 and min(turn, n_yaw - turn) <= 1:
                recovered += 1
        rows.append(row)
    return {"n_yaw": n_yaw, "poses_tried": len(rows), "poses_skipped": skipped, "poses_recovered": recovered, "rows": rows}


def scan_localize_text(result):
    """The text of map/scan_localize.txt: two header lines, one tab-separated row per pose tried in SCAN_ROW_ORDER, then
    `name<TAB>value` per summary value.  Numbers are written with repr(): reading the file gives them back bit for bit."""
    lines = [_SCAN_HEAD + ": a range scan cast at each pose of the run and found again by the exhaustive scan match in a "
             "window around it (how well a planar scanner tells the places of this map apart; exact to the cell and the "
             "yaw step 2 pi / n_yaw)", "\t".join(SCAN_ROW_ORDER)]
    for row in result["rows"]:
        lines.append("\t".join(repr(float(row[k]) if k in _SCAN_ROW_FLOATS else int(row[k])) for k in SCAN_ROW_ORDER))
    lines += [f"{k}\t{int(result[k])!r}" for k in SCAN_SUMMARY_ORDER]
    return "\n".join(lines) + "\n"


def parse_scan_localize(text):
    """scan_localize_text's inverse: the dict it was given."""
    lines = text.splitlines()
    n = len(lines) - 2 - len(SCAN_SUMMARY_ORDER)
    if n < 0 or not lines[0].startswith(_SCAN_HEAD) or lines[1].split("\t") != list(SCAN_ROW_ORDER):
        raise ValueError("not a map/scan_localize.txt")
    result = {"rows": []}
    for line in lines[2:2 + n]:
        values = line.split("\t")
        if len(values) != len(SCAN_ROW_ORDER):
            raise ValueError(f"scan_localize.txt: a row of {len(values)} values, {len(SCAN_ROW_ORDER)} are expected")
        result["rows"].append({k: float(s) if k in _SCAN_ROW_FLOATS else int(s) for k, s in zip(SCAN_ROW_ORDER, values)})
    for key, line in zip(SCAN_SUMMARY_ORDER, lines[2 + n:]):
        name, _, value = line.partition("\t")
        if name != key:
            raise ValueError(f"scan_localize.txt: expected {key}, found {name}")
        result[key] = int(value)
    return result
