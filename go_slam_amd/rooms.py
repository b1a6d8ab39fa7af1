"""Which rooms there are: the free space of a passability lattice split by clearance into rooms, the doorways between them
and the graph of both (csrc/rooms.hip).

Places wide enough to be a room's interior -- the 26-connected components of the `core` cells -- are seeds; every other
open cell joins the seed it is nearest to along a drivable route, ties to the lower root; where two such regions meet
there is a doorway.  `room_segments` runs it on the GPU: gs_room_mark and gs_frontier_relax label the cores,
`plan.geodesic_field`'s kernels seeded at every kept core cell give the cost, gs_room_relax carries the cores' labels
outward along shortest routes only, gs_room_door_mark and gs_frontier_relax label the doorways, and gs_room_table /
gs_room_door_table fold rooms and doorways into one row each.  Everything is integer and every relaxation has a unique
fixed point, so the result equals a serial restatement bit for bit (tests/rooms_restatement.py; include/goslam_hip.h,
gs_room_*).  `ESDF.rooms` (tsdf.py) puts a fused volume's distance field under it, `rooms_on_map`
two 2-D occupancy maps, and `rooms_text` / `parse_rooms` are the run's map/rooms.txt.
"""
import ast
import math

import numpy as np
import torch

from . import _lib
from . import plan as _plan

INF = _plan.INF                        # GS_GEO_INF
MAX_CELLS = _plan.MAX_CELLS            # per axis
SWEEP_BATCH = _plan.SWEEP_BATCH        # sweeps enqueued per host read of `changed`
ROOM_COLUMNS = ("root", "size", "core_size", "sum", "bbox", "reach")
DOOR_COLUMNS = ("root", "size", "sum", "bbox", "room_lo", "room_hi", "widest_cell", "widest_d2")


def _row_of(root, label):
    """The row of every label among the ascending `root` (torch.searchsorted), -1 where the label is none of them."""
    if int(root.shape[0]) == 0:
        return torch.full_like(label, -1)
    at = torch.searchsorted(root, label.contiguous()).clamp_(max=int(root.shape[0]) - 1).to(torch.int32)
    return torch.where(root[at.long()] == label, at, torch.full_like(at, -1))


class RoomSegments:
    """The rooms and doorways of a lattice.  On the device: `.label` int32 [n0,n1,n2] (the root of the cell's room, -1 off
    the rooms), `.room` int32 (the room's id, its row in the table; -1 off the rooms), `.cost` int32 (milli-voxels to the
    nearest kept core cell, INF where none is reachable), `.door_label` int32 (-1 off the doorways, else the smallest
    linear index of the cell's doorway), `.open` uint8 as given, `.counts` int64 [3] (open, core and boundary cells),
    `.rooms`, the room table, one row per kept core by ascending root: {"root", "size", "core_size", "reach" int32 [K],
    "sum" int64 [K,3], "bbox" int32 [K,6] (mins, then maxes)}, and `.doors`, one row per doorway by ascending root:
    {"root", "size", "room_lo", "room_hi" (labels), "room_a", "room_b" (their ids), "widest_cell", "widest_d2" int32 [D],
    "sum" int64 [D,3], "bbox" int32 [D,6]}.  A doorway where three rooms meet reports only the extremes of their labels:
    room_lo / room_a and room_hi / room_b.  widest_cell is the doorway's cell with the largest d2, ties to the lowest
    index (without d2: its root, and widest_d2 = 0).  `.n_rooms` = K, `.n_doors` = D, `.core_roots` / `.core_sizes` int32
    (every core component, kept or not), `.dims`, and `.sweeps`, the brick sweeps each of the four relaxations needed:
    {"cores", "cost", "rooms", "doors"} (they may differ between runs, the results do not)."""

    def __init__(self, open, label, cost, door_label, counts, rooms, doors, cores, sweeps):
        self.open, self.label, self.cost, self.door_label, self.counts = open, label, cost, door_label, counts
        self.rooms, self.doors, self.sweeps = rooms, doors, dict(sweeps)
        self.core_roots, self.core_sizes = cores
        self.n_rooms, self.n_doors = int(rooms["root"].shape[0]), int(doors["root"].shape[0])
        self.dims = tuple(int(n) for n in label.shape)
        self.device = label.device
        self.room = _row_of(rooms["root"], label)
        self._graph = None

    def graph(self):
        """The room graph, on the host: {"doors": [(room_a, room_b) per doorway], "rooms": [{"doors": [ids], "neighbours":
        [room ids, ascending]} per room]}.  One read of two columns, kept for later calls."""
        if self._graph is None:
            ends = torch.stack([self.doors["room_a"], self.doors["room_b"]], dim=1).cpu().tolist()
            rooms = [{"doors": [], "neighbours": set()} for _ in range(self.n_rooms)]
            for d, (a, b) in enumerate(ends):
                for here, there in ((a, b), (b, a)):
                    if here >= 0 and d not in rooms[here]["doors"]:
                        rooms[here]["doors"].append(d)
                    if here >= 0 and there >= 0 and there != here:
                        rooms[here]["neighbours"].add(there)
            self._graph = {"doors": [tuple(e) for e in ends],
                           "rooms": [{"doors": r["doors"], "neighbours": sorted(r["neighbours"])} for r in rooms]}
        return self._graph

    def rooms_along(self, cells):
        """What a path crosses: `cells` integers [L,3] (the "cells" of `ESDF.plan`'s dict; [L,2] map cells count as
        (0, u, v)) -> {"rooms": the ids of the rooms in the order the path is in them, "cells": the number of the path's
        cells in each (a run-length list: a room entered twice appears twice), "doors": the ids of the doorways it
        touches, in order, repeats in a row dropped}.  Cells off the rooms are skipped.  One read."""
        cells = torch.as_tensor(cells, device=self.device).long()
        if cells.dim() != 2 or int(cells.shape[1]) not in (2, 3):
            raise ValueError(f"RoomSegments.rooms_along: cells must be [L,3] (got {list(cells.shape)})")
        if int(cells.shape[1]) == 2:
            cells = torch.cat([torch.zeros_like(cells[:, :1]), cells], dim=1)
        if int(cells.shape[0]) == 0:
            return {"rooms": [], "cells": [], "doors": []}
        dims = torch.tensor(self.dims, device=self.device)
        if bool(((cells < 0) | (cells >= dims[None, :])).any()):
            raise ValueError(f"RoomSegments.rooms_along: a cell lies outside the lattice {self.dims}")
        i0, i1, i2 = cells[:, 0], cells[:, 1], cells[:, 2]
        door = _row_of(self.doors["root"], self.door_label[i0, i1, i2])
        room, door = torch.stack([self.room[i0, i1, i2], door]).cpu().tolist()                 # the one read
        out = {"rooms": [], "cells": [], "doors": []}
        for r, d in zip(room, door):
            if r >= 0:
                if out["rooms"] and out["rooms"][-1] == r:
                    out["cells"][-1] += 1
                else:
                    out["rooms"].append(r)
                    out["cells"].append(1)
            if d >= 0 and (not out["doors"] or out["doors"][-1] != d):
                out["doors"].append(d)
        return out

    def room_at(self, cell):
        """The id of the room of one cell (three integers), -1 off the rooms.  One 4-byte read."""
        c = _plan._cell(cell, self.dims, "RoomSegments.room_at")
        return int(self.room[c[0], c[1], c[2]].item())

    def centroid_cells(self, table=None):
        """float64 [K,3]: the mean coordinates of every room's cells (or of the rows of `table`, such as `.doors`)."""
        table = self.rooms if table is None else table
        return table["sum"].double() / table["size"].double()[:, None]


def segment_arguments(open, core, d2=None, min_core_cells=1, max_cost=None, max_sweeps=65536):
    """(dims, min_core_cells, max_cost, max_sweeps) of `room_segments`, or ValueError.  Touches no device."""
    what = "room_segments"
    for name, t in (("open", open), ("core", core)):
        if not isinstance(t, torch.Tensor) or t.dtype not in (torch.uint8, torch.bool):
            raise ValueError(f"{what}: {name} must be a uint8 or bool tensor (got {getattr(t, 'dtype', type(t).__name__)})")
    if open.dim() != 3 or not all(1 <= int(n) <= MAX_CELLS for n in open.shape):
        raise ValueError(f"{what}: open must be [n0,n1,n2] with every size in [1, {MAX_CELLS}] "
                         f"(got {list(open.shape)}); a 2-D map [n_u,n_v] is the lattice [1,n_u,n_v]")
    dims = tuple(int(n) for n in open.shape)
    if tuple(core.shape) != dims:
        raise ValueError(f"{what}: core is {list(core.shape)}, open is {list(dims)}")
    if d2 is not None:
        if not isinstance(d2, torch.Tensor) or d2.dtype != torch.int32:
            raise ValueError(f"{what}: d2 must be an int32 tensor or None (got {getattr(d2, 'dtype', type(d2).__name__)})")
        if tuple(d2.shape) != dims:
            raise ValueError(f"{what}: d2 is {list(d2.shape)}, open is {list(dims)}")
    if isinstance(min_core_cells, bool) or not isinstance(min_core_cells, (int, np.integer)) or int(min_core_cells) < 1:
        raise ValueError(f"{what}: min_core_cells must be a positive integer (got {min_core_cells!r})")
    if max_cost is None:
        max_cost = _plan.MAX_COST
    if isinstance(max_cost, bool) or not isinstance(max_cost, (int, np.integer)) or not 0 <= int(max_cost) <= _plan.MAX_COST:
        raise ValueError(f"{what}: max_cost must be an integer in [0, {_plan.MAX_COST}] milli-voxels (got {max_cost!r})")
    if isinstance(max_sweeps, bool) or not isinstance(max_sweeps, (int, np.integer)) or int(max_sweeps) < 1:
        raise ValueError(f"{what}: max_sweeps must be a positive integer (got {max_sweeps!r})")
    return dims, int(min_core_cells), int(max_cost), int(max_sweeps)


@torch.no_grad()
def room_segments(open, core, d2=None, min_core_cells=1, max_cost=None, max_sweeps=65536):
    """The rooms and doorways of the lattice `open` (uint8 or bool [n0,n1,n2], non-zero where the robot's centre may be;
    on the GPU, or moved there): a `RoomSegments`.  `core` (same shape) is non-zero where the robot has room to spare: the
    26-connected components of the cells that are both, those of at least `min_core_cells` cells, seed one room each.
    Every open cell a route of at most `max_cost` milli-voxels leads to from a kept core joins the core it is nearest to
    (the cost is `plan.geodesic_field`'s from every kept core cell), ties to the lower root.  `d2` (int32, same shape:
    `ESDF.d2`; None: 0 everywhere) finds every doorway's widest cell.  Each of the four relaxations is enqueued in batches
    of SWEEP_BATCH sweeps through `plan.sweep_to_fixed_point` and `changed` is read once per batch; RuntimeError when
    `max_sweeps` sweeps do not get one of them there.  Further host reads: the numbers of core components and of doorways
    (4 bytes each) and the numbers of kept cores and of their cells.  ValueError for bad shapes, dtypes or sizes, before
    the device is touched."""
    dims, min_core_cells, max_cost, max_sweeps = segment_arguments(open, core, d2, min_core_cells, max_cost, max_sweeps)
    what = "room_segments"
    L = _lib.lib()
    P = _lib.ptr
    dev = open.device if open.is_cuda else torch.device("cuda", torch.cuda.current_device())
    open = open.to(device=dev, dtype=torch.uint8).contiguous()
    core = core.to(device=dev, dtype=torch.uint8).contiguous()
    d2 = None if d2 is None else d2.to(dev).contiguous()
    label = torch.empty(dims, dtype=torch.int32, device=dev)
    door_label = torch.empty(dims, dtype=torch.int32, device=dev)
    counts = torch.empty(3, dtype=torch.int32, device=dev)                    # u32, each at most 2^30
    flags = torch.empty(L.gs_frontier_flags_bytes(*dims), dtype=torch.uint8, device=dev)
    changed = torch.empty(SWEEP_BATCH, dtype=torch.int32, device=dev)        # u32 0 / 1
    ws_bytes = L.gs_frontier_workspace_bytes(*dims)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    n_roots = torch.empty(1, dtype=torch.int32, device=dev)
    sweeps = {}

    def components(lab, stage, sizes):
        """gs_frontier_relax to the fixed point, then the ascending roots (and sizes) of the label lattice `lab`."""
        sweeps[stage] = _plan.sweep_to_fixed_point(
            lambda sweep0, k: _lib.check(L.gs_frontier_relax(*dims, P(lab), P(flags), sweep0, k, P(changed), stream),
                                         f"{what} ({stage}: relax)"), changed, max_sweeps, f"{what} ({stage})")
        _lib.check(L.gs_frontier_roots(P(lab), *dims, P(ws), ws_bytes, P(n_roots), stream), f"{what} ({stage}: roots)")
        n = int(n_roots.item())                                               # the read that sizes the table
        root = torch.empty(n, dtype=torch.int32, device=dev)
        size = torch.empty(n, dtype=torch.int32, device=dev) if sizes else None
        if n > 0:
            _lib.check(L.gs_room_cores(P(lab), *dims, P(ws), ws_bytes, n, n, P(root), P(size), stream),
                       f"{what} ({stage}: table)")
        return root, size

    with torch.cuda.device(dev):
        stream = _lib.stream_ptr(dev)
        _lib.check(L.gs_room_mark(P(open), P(core), *dims, P(label), P(counts), P(flags), stream), f"{what} (mark)")
        core_roots, core_sizes = components(label, "cores", True)
        keep = (core_sizes >= min_core_cells).to(torch.uint8)
        _lib.check(L.gs_room_seed(P(open), *dims, P(core_roots), P(keep), int(core_roots.shape[0]), P(label), P(flags),
                                  stream), f"{what} (seed)")
        root = core_roots[keep != 0].contiguous()                             # a read: the number of kept cores
        K = int(root.shape[0])
        # plan.geodesic_field's two calls, with the seeds (every kept core cell: millions in a large flat) left on the device
        seeds = torch.nonzero(label >= 0).to(torch.int32).contiguous()        # (nonzero's own layout is [3,m]); one read
        m = int(seeds.shape[0])
        cost = torch.empty(dims, dtype=torch.int32, device=dev)
        cost_flags = torch.empty(L.gs_geodesic_flags_bytes(*dims), dtype=torch.uint8, device=dev)
        _lib.check(L.gs_geodesic_init(P(open), *dims, P(seeds) if m else None, m, P(cost), P(cost_flags), stream),
                   f"{what} (cost: init)")
        sweeps["cost"] = _plan.sweep_to_fixed_point(
            lambda sweep0, k: _lib.check(L.gs_geodesic_relax(P(open), *dims, max_cost, P(cost), P(cost_flags), sweep0, k,
                                                             P(changed), stream), f"{what} (cost: relax)"),
            changed, max_sweeps, f"{what} (cost)")
        sweeps["rooms"] = _plan.sweep_to_fixed_point(
            lambda sweep0, k: _lib.check(L.gs_room_relax(P(open), P(cost), *dims, P(label), P(flags), sweep0, k, P(changed),
                                                         stream), f"{what} (rooms: relax)"),
            changed, max_sweeps, f"{what} (rooms)")
        _lib.check(L.gs_room_door_mark(P(open), P(label), *dims, P(door_label), P(counts[2:]), P(flags), stream),
                   f"{what} (door mark)")
        door_root, _ = components(door_label, "doors", False)
        D = int(door_root.shape[0])
        rooms = {"root": root, "size": torch.empty(K, dtype=torch.int32, device=dev),
                 "core_size": torch.empty(K, dtype=torch.int32, device=dev),
                 "sum": torch.empty((K, 3), dtype=torch.int64, device=dev),
                 "bbox": torch.empty((K, 6), dtype=torch.int32, device=dev),
                 "reach": torch.empty(K, dtype=torch.int32, device=dev)}
        doors = {"root": door_root, "size": torch.empty(D, dtype=torch.int32, device=dev),
                 "sum": torch.empty((D, 3), dtype=torch.int64, device=dev),
                 "bbox": torch.empty((D, 6), dtype=torch.int32, device=dev),
                 "room_lo": torch.empty(D, dtype=torch.int32, device=dev),
                 "room_hi": torch.empty(D, dtype=torch.int32, device=dev)}
        widest = torch.empty((D, 2), dtype=torch.int32, device=dev)           # one u64 key per row: (~cell, d2)
        if K > 0:
            _lib.check(L.gs_room_table(P(label), P(cost), *dims, P(root), K, P(rooms["size"]), P(rooms["core_size"]),
                                       P(rooms["sum"]), P(rooms["bbox"]), P(rooms["reach"]), stream), f"{what} (room table)")
        if D > 0:
            _lib.check(L.gs_room_door_table(P(open), P(label), P(door_label), P(d2), *dims, P(door_root), D,
                                            P(doors["size"]), P(doors["sum"]), P(doors["bbox"]), P(doors["room_lo"]),
                                            P(doors["room_hi"]), P(widest), stream), f"{what} (door table)")
    doors["widest_cell"], doors["widest_d2"] = -1 - widest[:, 0], widest[:, 1]      # 0xffffffff - cell as int32 is -1 - cell
    doors["room_a"], doors["room_b"] = _row_of(root, doors["room_lo"]), _row_of(root, doors["room_hi"])
    return RoomSegments(open, label, cost, door_label, counts.long(), rooms, doors, (core_roots, core_sizes), sweeps)


def _map_cells(grid, what, name):
    cells = grid["cells"]
    cells = cells if isinstance(cells, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(cells))
    if cells.dim() != 2 or cells.dtype != torch.uint8:
        raise ValueError(f"{what}: {name}'s cells must be uint8 [n_u,n_v] (got {cells.dtype} {list(cells.shape)})")
    res = float(grid["resolution"])
    if not res > 0:
        raise ValueError(f"{what}: {name}'s resolution must be positive (got {res})")
    return cells, res, [float(v) for v in grid["origin"]]


@torch.no_grad()
def rooms_on_map(grid, core_grid, min_core_cells=1):
    """The rooms of a 2-D map: `grid` and `core_grid` are two dicts of `ESDF.occupancy_slice` or `load_map` (cells uint8
    [n_u,n_v], origin, resolution) of the same shape, origin and resolution, the first made with the robot's radius, the
    second with the larger radius that marks a room's interior.  A cell is open where `grid` is free (254) and core where
    `core_grid` is: a `RoomSegments` over the lattice [1,n_u,n_v] with the extras `.area_m2` float64 [K] = size *
    resolution^2, `.centroid` float64 [K,2] = origin + (centroid_cells[:, 1:] + 0.5) * resolution and `.door_centre`
    float64 [D,2], the same of every doorway's widest_cell (no d2 here: its root).  ValueError when the two maps
    disagree, before the device is touched."""
    what = "rooms_on_map"
    cells, res, origin = _map_cells(grid, what, "grid")
    core_cells, core_res, core_origin = _map_cells(core_grid, what, "core_grid")
    if tuple(cells.shape) != tuple(core_cells.shape) or res != core_res or origin != core_origin:
        raise ValueError(f"{what}: the two maps disagree: {list(cells.shape)} at {origin} by {res} and "
                         f"{list(core_cells.shape)} at {core_origin} by {core_res}")
    open = (cells == _plan.MAP_FREE)[None].contiguous()
    core = (core_cells == _plan.MAP_FREE)[None].to(open.device).contiguous()
    out = room_segments(open, core, None, min_core_cells)
    o = torch.tensor(origin, dtype=torch.float64, device=out.device)[None, :]
    out.area_m2 = out.rooms["size"].double() * res ** 2
    out.centroid = o + (out.centroid_cells()[:, 1:] + 0.5) * res
    w = out.doors["widest_cell"].long()
    n_v = out.dims[2]
    out.door_centre = o + (torch.stack([w // n_v, w % n_v], dim=1).double() + 0.5) * res
    return out


# ---- map/rooms.txt ------------------------------------------------------------------------------------------------------
SUMMARY_ORDER = ("n_open", "n_core", "n_boundary", "n_rooms", "n_doors", "object_rooms", "along_rooms", "along_doors",
                 "camera_room")
ROOM_TEXT_INTS = ("id", "root", "size", "core_size", "reach", "min0", "min1", "min2", "max0", "max1", "max2")
ROOM_TEXT_FLOATS = ("centroid_x", "centroid_y", "centroid_z", "volume_m3", "lo_x", "lo_y", "lo_z", "hi_x", "hi_y", "hi_z")
DOOR_TEXT_INTS = ("id", "root", "size", "room_a", "room_b", "widest_cell", "widest_d2")
DOOR_TEXT_FLOATS = ("centre_x", "centre_y", "centre_z", "width_m", "centroid_x", "centroid_y", "centroid_z")
_HEADER = "Rooms of the fused TSDF volume"


def object_rooms(result, objects):
    """The room id of every box of `objects` (the boxes of `find_objects`, or an `Objects`, in the frame of the field
    `result` came from): the room of the open cell nearest the box's centre (`plan.snap_cell` within the box's largest
    half extent), -1 when there is none or it lies in no room."""
    boxes = objects.boxes if hasattr(objects, "boxes") else objects
    out = []
    for b in boxes:
        centre = np.asarray(b["centre"], np.float64)
        cell = [int(math.floor((centre[a] - result.lo[a]) / result.voxel + 0.5)) for a in range(3)]
        at = _plan.snap_cell(result.open, cell, 0.5 * float(np.max(np.asarray(b["size_m"], np.float64))) / result.voxel)
        out.append(-1 if at is None else result.room_at(at))
    return out


def room_of_point(result, point, snap=0.0):
    """The id of the room of the world point `point` on the `RoomSegments` of `ESDF.rooms`: that of its nearest lattice
    point, moved by up to `snap` metres to an open cell (`plan.snap_cell`); -1 when there is none or it lies in no room."""
    cell = [int(math.floor((float(point[a]) - result.lo[a]) / result.voxel + 0.5)) for a in range(3)]
    at = _plan.snap_cell(result.open, cell, float(snap) / result.voxel)
    return -1 if at is None else result.room_at(at)


def config_arguments(opt, voxel, max_distance=None):
    """The checked values of cfg["tsdf"]["esdf"]["rooms"]: {"robot_radius", "core_radius", "min_core_m3" (or None), "snap"},
    or ValueError.  `max_distance` is tsdf.esdf.max_distance, the band of the field to come (None: unbounded)."""
    what = "fuse_from_config: tsdf.esdf.rooms"
    out = {}
    for key, default in (("robot_radius", 0.0), ("core_radius", 0.6), ("min_core_m3", None), ("snap", 0.0)):
        v = opt.get(key, default)
        if v is not None:
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v):
                raise ValueError(f"{what}.{key} must be a finite number (got {v!r})")
            v = float(v)
        out[key] = v
    unknown = sorted(set(opt) - {"enable", "robot_radius", "core_radius", "min_core_m3", "snap"})
    if unknown:
        raise ValueError(f"{what}: unknown keys {unknown}")
    band = math.inf if max_distance is None else math.ceil(float(max_distance) / voxel) * voxel
    if not 0 <= out["robot_radius"] < out["core_radius"] <= band:
        raise ValueError(f"{what}: need 0 <= robot_radius < core_radius <= {band} m, the field's band "
                         f"(got {out['robot_radius']} and {out['core_radius']})")
    if out["min_core_m3"] is not None and not out["min_core_m3"] > 0:
        raise ValueError(f"{what}.min_core_m3 must be positive (got {out['min_core_m3']})")
    if not out["snap"] >= 0:
        raise ValueError(f"{what}.snap must be a distance >= 0 in metres (got {out['snap']})")
    return out


def summary(result, objects=None, along=None, camera_room=None):
    """The dict `rooms_text` writes, from the `RoomSegments` of `ESDF.rooms` (with its world-space extras), the objects
    (see `object_rooms`) or None, `rooms_along`'s dict of a path or None and the room the camera is in (`room_of_point`)
    or None.  One read of the counts and the tables."""
    counts = [int(v) for v in result.counts.cpu().tolist()]
    r, d = result.rooms, result.doors
    K, D = result.n_rooms, result.n_doors

    def col(t, dtype):
        return t.cpu().numpy().astype(dtype)
    rooms = {"id": np.arange(K, dtype=np.int64), "root": col(r["root"], np.int64), "size": col(r["size"], np.int64),
             "core_size": col(r["core_size"], np.int64), "reach": col(r["reach"], np.int64)}
    bbox = col(r["bbox"], np.int64).reshape(K, 6)
    for j, name in enumerate(ROOM_TEXT_INTS[5:]):
        rooms[name] = bbox[:, j]
    world = np.concatenate([col(result.centroid, np.float64).reshape(K, 3), col(result.volume_m3, np.float64).reshape(K, 1),
                            col(result.box_lo, np.float64).reshape(K, 3), col(result.box_hi, np.float64).reshape(K, 3)],
                           axis=1)
    for j, name in enumerate(ROOM_TEXT_FLOATS):
        rooms[name] = world[:, j]
    doors = {"id": np.arange(D, dtype=np.int64)}
    for name in DOOR_TEXT_INTS[1:]:
        doors[name] = col(d[name], np.int64)
    world = np.concatenate([col(result.door_centre, np.float64).reshape(D, 3),
                            col(result.door_width_m, np.float64).reshape(D, 1),
                            col(result.door_centroid, np.float64).reshape(D, 3)], axis=1)
    for j, name in enumerate(DOOR_TEXT_FLOATS):
        doors[name] = world[:, j]
    return {"n_open": counts[0], "n_core": counts[1], "n_boundary": counts[2], "n_rooms": K, "n_doors": D,
            "object_rooms": None if objects is None else [int(v) for v in object_rooms(result, objects)],
            "along_rooms": None if along is None else [int(v) for v in along["rooms"]],
            "along_doors": None if along is None else [int(v) for v in along["doors"]],
            "camera_room": None if camera_room is None else int(camera_room), "rooms": rooms, "doors": doors}


def rooms_text(result, objects=None, along=None, camera_room=None):
    """The text of map/rooms.txt for the `RoomSegments` of `ESDF.rooms` (or `summary`'s dict of one): two header lines,
    `name<TAB>repr(value)` for the SUMMARY_ORDER keys, then one line per room and one per doorway, every number written
    with repr(): `parse_rooms` gives them back bit for bit.  With `objects` (the boxes of `find_objects`, already in the
    frame of the field) object_rooms lists the room of each, see `object_rooms`; with `along` (`rooms_along`'s dict of a
    path) along_rooms and along_doors list what the path crosses, and camera_room is `room_of_point`'s answer or None."""
    report = result if isinstance(result, dict) else summary(result, objects, along, camera_room)
    lines = [_HEADER + "'s distance field: the free space split by clearance into rooms and the doorways between them",
             "(object_rooms: the room of every object of map/objects.txt, or None; along_rooms / along_doors: the rooms and "
             "doorways along map/path.txt, or None; camera_room: the room the last camera centre is in, or None; then per "
             "room: " + " ".join(ROOM_TEXT_INTS + ROOM_TEXT_FLOATS) + "; then per doorway: "
             + " ".join(DOOR_TEXT_INTS + DOOR_TEXT_FLOATS) + "; width_m = 2 sqrt(widest_d2) voxel)"]
    lines += [f"{k}\t{report[k]!r}" for k in SUMMARY_ORDER]
    for table, ints, floats in ((report["rooms"], ROOM_TEXT_INTS, ROOM_TEXT_FLOATS),
                                (report["doors"], DOOR_TEXT_INTS, DOOR_TEXT_FLOATS)):
        for i in range(len(table["id"])):
            lines.append(" ".join([repr(int(table[c][i])) for c in ints] + [repr(float(table[c][i])) for c in floats]))
    return "\n".join(lines) + "\n"


def parse_rooms(text):
    """rooms_text's inverse: `summary`'s dict, the tables' columns as int64 or float64 arrays."""
    lines = text.splitlines()
    if len(lines) < 2 + len(SUMMARY_ORDER) or not lines[0].startswith(_HEADER):
        raise ValueError("not a map/rooms.txt")
    result = {}
    for key, line in zip(SUMMARY_ORDER, lines[2:]):
        name, value = line.split("\t")
        if name != key:
            raise ValueError(f"rooms.txt: expected {key}, found {name}")
        try:
            result[key] = ast.literal_eval(value)
        except (ValueError, SyntaxError):
            raise ValueError(f"rooms.txt: {key} is {value!r}") from None
    at = 2 + len(SUMMARY_ORDER)
    if len(lines) != at + result["n_rooms"] + result["n_doors"]:
        raise ValueError("rooms.txt: the rows do not match n_rooms and n_doors")
    for key, n, ints, floats in (("rooms", result["n_rooms"], ROOM_TEXT_INTS, ROOM_TEXT_FLOATS),
                                 ("doors", result["n_doors"], DOOR_TEXT_INTS, DOOR_TEXT_FLOATS)):
        rows = [line.split(" ") for line in lines[at:at + n]]
        if any(len(r) != len(ints) + len(floats) for r in rows):
            raise ValueError(f"rooms.txt: a row of {key} does not have {len(ints) + len(floats)} columns")
        result[key] = {c: np.array([int(r[j]) for r in rows], dtype=np.int64).reshape(n) for j, c in enumerate(ints)}
        result[key].update({c: np.array([float(r[len(ints) + j]) for r in rows], dtype=np.float64).reshape(n)
                            for j, c in enumerate(floats)})
        at += n
    return result
