"""Where the floor carries a robot: the elevation and traversability map of a fused volume's state lattice
(csrc/floor.hip; include/goslam_hip.h, gs_floor_*; tests/floor_restatement.py).

`columns` finds, per column of the lattice along the up axis, the lowest place in a band of heights where a base of a
given headroom can rest on seen support (`floor`, the lattice index, and `kind`: 0 never observed, 1 a floor with free
headroom, 2 a floor whose headroom was not seen solid but not all seen free either, 3 no floor: a wall, too low, a hole).
`footprint` lays the robot's disc on that elevation map: a column is drivable (254) when every column under the disc is a
kind-1 floor within `S` cells of its own height, occupied (0) when the disc meets a column without floor or a step above
`S`, else unknown (205).  Both are integer kernels, bit-exact against the restatement.  `ESDF.floor_map` (tsdf.py) is the
one call in metres; its dict has the shape of `ESDF.occupancy_slice`'s, so `plan_on_map`, `frontiers_on_map`,
`rooms_on_map`, `next_view_on_map` and `save_map` take it as it is.  `lift` puts a route planned on the map back on the
floor in 3-D, and `summary` with `floor_text` / `parse_floor` is the run's map/floor.txt.
"""
import math

import numpy as np
import torch

from . import _lib
from . import plan as _plan

MAX_CELLS = _plan.MAX_CELLS            # per axis
MAP_FREE, MAP_OCCUPIED, MAP_UNKNOWN = 254, 0, 205
R2_MIN, R2_MAX = 2, 32 * 32            # the disc holds the eight neighbours; the halo of a tile is at most 32 cells
KIND_UNSEEN, KIND_FLOOR, KIND_MAYBE, KIND_NONE = 0, 1, 2, 3
WHY_NONE, WHY_NO_FLOOR, WHY_NEAR_NO_FLOOR, WHY_STEP = 0, 1, 2, 3
H_MAX = 1 << 30                        # any headroom beyond the lattice's top acts alike


def _integer(value, name, what):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)):
        raise ValueError(f"{what}: {name} must be an integer (got {value!r})")
    return int(value)


def _axis_sign(up_axis, up_sign, what):
    if isinstance(up_axis, bool) or not isinstance(up_axis, (int, np.integer)) or not 0 <= int(up_axis) <= 2:
        raise ValueError(f"{what}: up_axis must be 0, 1 or 2 (got {up_axis!r})")
    if isinstance(up_sign, bool) or not isinstance(up_sign, (int, np.integer)) or int(up_sign) not in (1, -1):
        raise ValueError(f"{what}: up_sign must be +1 or -1 (got {up_sign!r})")
    return int(up_axis), int(up_sign)


def _image(t, name, dtype, shape, what):
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or (shape is not None and tuple(t.shape) != tuple(shape)) \
            or t.dim() != 2 or not all(2 <= int(n) <= MAX_CELLS for n in t.shape):
        want = "[n_u,n_v] with both sizes in [2, 1024]" if shape is None else str(list(shape))
        raise ValueError(f"{what}: {name} must be a {str(dtype).replace('torch.', '')} tensor {want} "
                         f"(got {getattr(t, 'dtype', type(t).__name__)} {list(getattr(t, 'shape', []))})")
    return t


def _outputs(out, specs, dev, what):
    """The output tensors: new ones, or the tuple `out` checked against (name, dtype, shape) of `specs`."""
    if out is None:
        return tuple(torch.empty(shape, dtype=dtype, device=dev) for _, dtype, shape in specs)
    if not isinstance(out, (tuple, list)) or len(out) != len(specs):
        raise ValueError(f"{what}: out must be the {len(specs)} tensors ({', '.join(s[0] for s in specs)})")
    for t, (name, dtype, shape) in zip(out, specs):
        _image(t, f"out {name}", dtype, shape, what)
        if t.device != dev or not t.is_contiguous():
            raise ValueError(f"{what}: out {name} must be contiguous on {dev}")
    return tuple(out)


def _on_gpu(t, name, what):
    if not t.is_cuda:
        raise ValueError(f"{what}: {name} must be on a GPU (it is on {t.device}); there is no host path")


@torch.no_grad()
def columns(state, up_axis, up_sign, p0, p1, H, out=None):
    """gs_floor_columns over state uint8 [nx,ny,nz] (0 unseen, 1 free, 2 solid; `ESDF.state`): per column along `up_axis`
    the lowest stand with its position in [p0, p1] under a headroom of H cells.  Positions count upward: the lattice index
    for up_sign +1, n - 1 - index for -1.  -> (floor int16 [n_u,n_v], the lattice index of the stand cell or -1; kind
    uint8 [n_u,n_v]) on the state's device, (u, v) the two other axes in increasing order; `out` = (floor, kind) writes
    into given tensors.  Enqueues on the current stream and reads nothing back.  ValueError before the device is touched."""
    what = "floor.columns"
    if not isinstance(state, torch.Tensor) or state.dtype != torch.uint8 or state.dim() != 3 \
            or not all(2 <= int(n) <= MAX_CELLS for n in state.shape):
        raise ValueError(f"{what}: state must be a uint8 tensor [nx,ny,nz] with every size in [2, 1024] "
                         f"(got {getattr(state, 'dtype', type(state).__name__)} {list(getattr(state, 'shape', []))})")
    a, sign = _axis_sign(up_axis, up_sign, what)
    p0, p1, H = _integer(p0, "p0", what), _integer(p1, "p1", what), _integer(H, "H", what)
    dims = tuple(int(n) for n in state.shape)
    if not 0 <= p0 <= p1 < dims[a]:
        raise ValueError(f"{what}: the band [{p0}, {p1}] must lie in [0, {dims[a] - 1}], the positions of axis {a}")
    if H < 1:
        raise ValueError(f"{what}: the headroom H must be at least one cell (got {H})")
    _on_gpu(state, "state", what)
    dev = state.device
    u, v = [ax for ax in range(3) if ax != a]
    shape = (dims[u], dims[v])
    floor, kind = _outputs(out, (("floor", torch.int16, shape), ("kind", torch.uint8, shape)), dev, what)
    state = state.contiguous()
    with torch.cuda.device(dev):
        rc = _lib.lib().gs_floor_columns(_lib.ptr(state), *dims, a, sign, p0, p1, min(H, H_MAX), _lib.ptr(floor),
                                         _lib.ptr(kind), _lib.stream_ptr(dev))
    _lib.check(rc, what)
    return floor, kind


@torch.no_grad()
def footprint(floor, kind, R2, S, out=None):
    """gs_floor_footprint over `columns`' maps: the disc of the offsets with du^2 + dv^2 <= R2 (2 <= R2 <= 1024), S >= 0
    the largest height difference in cells under it.  -> (cells uint8: 254 drivable, 0 occupied, 205 unknown; why uint8: 0,
    or for an occupied column 1 no floor here, 2 a column without floor under the disc, 3 a step above S; rough int16, the
    largest height difference under the disc), all [n_u,n_v]; `out` = (cells, why, rough) writes into given tensors.
    Enqueues on the current stream and reads nothing back.  ValueError before the device is touched."""
    what = "floor.footprint"
    _image(floor, "floor", torch.int16, None, what)
    _image(kind, "kind", torch.uint8, tuple(floor.shape), what)
    R2, S = _integer(R2, "R2", what), _integer(S, "S", what)
    if not R2_MIN <= R2 <= R2_MAX:
        raise ValueError(f"{what}: R2 must lie in [{R2_MIN}, {R2_MAX}] squared cells (got {R2})")
    if S < 0:
        raise ValueError(f"{what}: S must be >= 0 cells (got {S})")
    _on_gpu(floor, "floor", what)
    dev = floor.device
    if kind.device != dev:
        raise ValueError(f"{what}: kind must be on {dev} like floor (it is on {kind.device})")
    shape = tuple(int(n) for n in floor.shape)
    cells, why, rough = _outputs(out, (("cells", torch.uint8, shape), ("why", torch.uint8, shape),
                                       ("rough", torch.int16, shape)), dev, what)
    floor, kind = floor.contiguous(), kind.contiguous()
    with torch.cuda.device(dev):
        rc = _lib.lib().gs_floor_footprint(_lib.ptr(floor), _lib.ptr(kind), shape[0], shape[1], R2, S, _lib.ptr(cells),
                                           _lib.ptr(why), _lib.ptr(rough), _lib.stream_ptr(dev))
    _lib.check(rc, what)
    return cells, why, rough


def _metres(value, name, what, positive=False):
    if isinstance(value, bool) or not isinstance(value, (int, float, np.integer, np.floating)):
        raise ValueError(f"{what}: {name} must be a number of metres (got {value!r})")
    value = float(value)
    if not math.isfinite(value) or value < 0 or (positive and value <= 0):
        raise ValueError(f"{what}: {name} must be finite and {'positive' if positive else '>= 0'} (got {value})")
    return value


def robot_arguments(voxel, robot_radius, robot_height, step_height, what="ESDF.floor_map"):
    """(H, S, R2) of the kernels for a robot in metres on a lattice of `voxel` metres: H = ceil(robot_height / voxel)
    cells of headroom, S = floor(step_height / voxel) cells of step, R2 = floor((robot_radius / voxel)^2).  ValueError for
    a value that is not finite or negative, a height that is not positive, or a radius whose R2 leaves [2, 1024] (the
    message names the smallest and the largest usable radius).  Touches no device."""
    voxel = float(voxel)
    robot_radius = _metres(robot_radius, "robot_radius", what)
    robot_height = _metres(robot_height, "robot_height", what, positive=True)
    step_height = _metres(step_height, "step_height", what)
    R2 = int(math.floor((robot_radius / voxel) ** 2))
    if not R2_MIN <= R2 <= R2_MAX:
        raise ValueError(f"{what}: robot_radius {robot_radius} m is {R2} squared cells of {voxel} m, outside "
                         f"[{R2_MIN}, {R2_MAX}]: the smallest usable radius is sqrt(2) cells, {math.sqrt(2.0) * voxel!r} m (the "
                         f"disc must hold the eight neighbours), and a usable one lies below {math.sqrt(R2_MAX + 1.0) * voxel!r} m")
    H = int(min(math.ceil(robot_height / voxel), H_MAX))
    S = int(min(math.floor(step_height / voxel), MAX_CELLS))
    return max(H, 1), S, R2


def floor_heights(floor, lo, voxel, up_sign):
    """float32 like `floor`: the world coordinate along up of the lower face of the stand cells with the lattice indices
    `floor`, lo + (k - 0.5) * voxel for up_sign +1 and lo + (k + 0.5) * voxel for -1; NaN where floor < 0."""
    h = float(lo) + (floor.double() - 0.5 * up_sign) * float(voxel)
    return torch.where(floor >= 0, h, torch.full_like(h, math.nan)).float()


@torch.no_grad()
def lift(grid, cells):
    """The world points float64 [L,3] standing on the floor at the map cells `cells` [L,2] (u, v), e.g. the "cells" of
    `plan_on_map` on the floor-map dict `grid` of `ESDF.floor_map`: the cell's centre along the two image axes,
    "floor_height" along the up axis.  A torch gather on the map's device and one small read for the check.  ValueError
    for cells that are no integers [L,2], lie outside the map or have no floor."""
    what = "floor.lift"
    for key in ("floor_height", "origin", "resolution", "axes", "up_axis"):
        if not isinstance(grid, dict) or key not in grid:
            raise ValueError(f"{what}: grid must be the dict of ESDF.floor_map (no {key!r})")
    height = grid["floor_height"]
    dev = height.device
    if isinstance(cells, torch.Tensor):
        if cells.dim() != 2 or cells.shape[1] != 2 or cells.is_floating_point() or cells.dtype == torch.bool:
            raise ValueError(f"{what}: cells must be integers [L,2] (got {cells.dtype} {list(cells.shape)})")
        cells = cells.to(dev).long()
    else:
        c = np.asarray(cells)
        c = np.zeros((0, 2), dtype=np.int64) if c.size == 0 else c
        if c.ndim != 2 or c.shape[1] != 2 or not np.issubdtype(c.dtype, np.integer):
            raise ValueError(f"{what}: cells must be integers [L,2] (got {c.dtype} {list(c.shape)})")
        cells = torch.from_numpy(np.ascontiguousarray(c, dtype=np.int64)).to(dev)
    out = torch.zeros((int(cells.shape[0]), 3), dtype=torch.float64, device=dev)
    if cells.shape[0] == 0:
        return out
    n_u, n_v = (int(n) for n in height.shape)
    inside = (cells[:, 0] >= 0) & (cells[:, 0] < n_u) & (cells[:, 1] >= 0) & (cells[:, 1] < n_v)
    h = height[cells[:, 0].clamp(0, n_u - 1), cells[:, 1].clamp(0, n_v - 1)].double()
    bad = (~inside | torch.isnan(h)).nonzero()[:1].cpu().tolist()                          # the one read
    if bad:
        i = bad[0][0]
        raise ValueError(f"{what}: cell {i} of the route, {cells[i].cpu().tolist()}, "
                         + ("has no floor" if bool(inside[i]) else f"lies outside the map {[n_u, n_v]}"))
    res = float(grid["resolution"])
    u_ax, v_ax = (int(ax) for ax in grid["axes"])
    out[:, u_ax] = float(grid["origin"][0]) + (cells[:, 0].double() + 0.5) * res
    out[:, v_ax] = float(grid["origin"][1]) + (cells[:, 1].double() + 0.5) * res
    out[:, int(grid["up_axis"])] = h
    return out


FLOOR_REPORT_ORDER = ("drivable_m2", "blocked_m2", "unknown_m2", "blocked_no_floor", "blocked_near_no_floor",
                      "blocked_step", "floor_min_m", "floor_max_m", "rough_max_cells")
_FLOOR_COUNTS = ("blocked_no_floor", "blocked_near_no_floor", "blocked_step", "rough_max_cells")


@torch.no_grad()
def summary(grid):
    """The dict `floor_text` writes, from the dict of `ESDF.floor_map`: the drivable (254), blocked (0) and unknown (205)
    area in m^2, the blocked columns by their `why` code (1 no floor, 2 a column without floor under the disc, 3 a step),
    the smallest and the largest "floor_height" over the drivable columns (nan without one) and the largest "rough" among
    them, in cells.  One read."""
    cells, why, rough, height = grid["cells"], grid["why"], grid["rough"], grid["floor_height"].double()
    free = cells == MAP_FREE
    inf = torch.full_like(height, math.inf)
    row = torch.stack([free.sum().double(), (cells == MAP_OCCUPIED).sum().double(), (cells == MAP_UNKNOWN).sum().double(),
                       (why == WHY_NO_FLOOR).sum().double(), (why == WHY_NEAR_NO_FLOOR).sum().double(),
                       (why == WHY_STEP).sum().double(), torch.where(free, height, inf).min(),
                       torch.where(free, height, -inf).max(),
                       torch.where(free, rough, torch.zeros_like(rough)).max().double()]).cpu().tolist()   # the one read
    area = float(grid["resolution"]) ** 2
    any_free = row[0] > 0
    return {"drivable_m2": row[0] * area, "blocked_m2": row[1] * area, "unknown_m2": row[2] * area,
            "blocked_no_floor": int(row[3]), "blocked_near_no_floor": int(row[4]), "blocked_step": int(row[5]),
            "floor_min_m": row[6] if any_free else math.nan, "floor_max_m": row[7] if any_free else math.nan,
            "rough_max_cells": int(row[8])}


def floor_text(result):
    """The text of map/floor.txt: two header lines, then `name<TAB>value` per reported value of `summary`, written with
    repr() so that reading the file gives back the numbers bit for bit."""
    lines = ["Drivable floor of the fused TSDF volume: where the robot's base finds seen support with free headroom and no "
             "step above its limit under its footprint (areas [m^2] of the map's drivable, blocked and unknown columns)",
             "(blocked_*: blocked columns without a floor, with such a column under the footprint, with a step above the "
             "limit; floor_min_m, floor_max_m: the floor's height over the drivable columns, nan without one; "
             "rough_max_cells: the largest height difference under a drivable footprint)"]
    lines += [f"{k}\t{(int(result[k]) if k in _FLOOR_COUNTS else float(result[k]))!r}" for k in FLOOR_REPORT_ORDER]
    return "\n".join(lines) + "\n"


def parse_floor(text):
    """floor_text's inverse: the reported dict."""
    lines = text.splitlines()
    if len(lines) != 2 + len(FLOOR_REPORT_ORDER) or not lines[0].startswith("Drivable floor of the fused TSDF volume"):
        raise ValueError("not a map/floor.txt")
    result = {}
    for key, line in zip(FLOOR_REPORT_ORDER, lines[2:]):
        name, _, value = line.partition("\t")
        if name != key:
            raise ValueError(f"floor.txt: expected {key}, found {name}")
        result[key] = int(value) if key in _FLOOR_COUNTS else float(value)
    return result


def floor_config(value, voxel, what="fuse_from_config: tsdf.esdf.floor"):
    """None when the config value (absent, or {enable, up_axis, up_sign, height, robot_radius, robot_height, step_height,
    plan}) leaves the floor map off, else the checked {"up_axis", "up_sign", "height", "robot_radius", "robot_height",
    "step_height", "plan"}; ValueError for an unknown key, a missing or bad value, or a robot that `robot_arguments`
    refuses on a lattice of `voxel` metres.  Touches no device."""
    if value is None:
        return None
    keys = {"enable", "up_axis", "up_sign", "height", "robot_radius", "robot_height", "step_height", "plan"}
    if not isinstance(value, dict) or set(value) - keys:
        raise ValueError(f"{what} must be a dict with keys among {sorted(keys)} (got {value!r})")
    for key in ("enable", "plan"):
        if not isinstance(value.get(key, False), bool):
            raise ValueError(f"{what}.{key} must be a bool (got {value[key]!r})")
    if not value.get("enable", False):
        return None
    missing = sorted(k for k in ("up_axis", "height", "robot_radius", "robot_height", "step_height") if k not in value)
    if missing:
        raise ValueError(f"{what}: missing {missing}")
    a, sign = _axis_sign(value["up_axis"], value.get("up_sign", 1), what)
    try:
        h0, h1 = (float(h) for h in value["height"])
    except (TypeError, ValueError):
        raise ValueError(f"{what}.height must be (h0, h1) in metres (got {value['height']!r})") from None
    if math.isnan(h0) or math.isnan(h1) or h0 > h1:
        raise ValueError(f"{what}.height must be (h0, h1) with h0 <= h1 (got {value['height']!r})")
    robot_arguments(voxel, value["robot_radius"], value["robot_height"], value["step_height"], what)
    return {"up_axis": a, "up_sign": sign, "height": (h0, h1), "robot_radius": float(value["robot_radius"]),
            "robot_height": float(value["robot_height"]), "step_height": float(value["step_height"]),
            "plan": value.get("plan", False)}
