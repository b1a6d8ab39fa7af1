"""Collision-free paths over a passability lattice: the cost-to-go field and the path walked down it (csrc/geodesic.hip).

`geodesic_field` relaxes, brick by brick on the GPU, the length of the shortest route from every passable cell to a set
of seed cells -- 26 moves of 1000 / 1414 / 1732 milli-voxels that cut no corner -- and `GeodesicField.path` walks from a
cell down to a seed.  The field is integer and the unique fixed point of its relaxation, so it equals a serial Dijkstra
bit for bit (tests/geodesic_restatement.py; include/goslam_hip.h, gs_geodesic_*).
`ESDF.passable` / `plan` / `reachable` (tsdf.py) put a fused volume's distance field under it, `plan_on_map` a 2-D
occupancy map, and `path_text` / `parse_path` are the run's map/path.txt.

`line_of_sight`, `segment_min` and `straighten` (csrc/sight.hip; include/goslam_hip.h, gs_segment_* / gs_path_*;
tests/sight_restatement.py) turn such a chain of lattice cells into the few waypoints a controller
wants: the shortest route over the path's own cells whose straight legs the robot may take.  `with_waypoints` is the one
helper behind the `straighten=True` of `ESDF.plan`, `explore`, `next_view` and `plan_on_map`, and `straight_path_text` /
`parse_straight_path` are the run's map/path_straight.txt.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib

INF = 0x3fffffff                       # GS_GEO_INF
MAX_COST = INF - 1732                  # GS_GEO_MAX_COST
MAX_CELLS = 1024                       # per axis
SWEEP_BATCH = 8                        # sweeps enqueued per host read of `changed`
MAP_FREE, MAP_UNKNOWN = 254, 205       # tsdf.MAP_FREE, tsdf.MAP_UNKNOWN
PATH_MAX_CELLS = 16384                 # GS_PATH_MAX_CELLS
DEFAULT_WINDOW = 256                   # earlier cells a path cell is tested against


def _cell(cell, dims, what):
    try:
        c = [int(v) for v in (cell.tolist() if hasattr(cell, "tolist") else cell)]
    except (TypeError, ValueError):
        c = None
    if c is None or len(c) != 3:
        raise ValueError(f"{what}: a cell is three integers (got {cell!r})")
    if not all(0 <= c[i] < dims[i] for i in range(3)):
        raise ValueError(f"{what}: cell {tuple(c)} lies outside the lattice {tuple(dims)}")
    return c


class GeodesicField:
    """A cost-to-go field at its fixed point: `.cost` int32 [n0,n1,n2] in milli-voxels (INF = 0x3fffffff where no seed
    is reachable within the cap), `.passable` uint8 [n0,n1,n2] it was built over, `.dims`, and `.sweeps`, the number of
    brick sweeps that were needed (the last of them lowered nothing; it may differ between runs, the field does not)."""

    def __init__(self, cost, passable, sweeps):
        self.cost, self.passable, self.sweeps = cost, passable, int(sweeps)
        self.dims = tuple(int(n) for n in cost.shape)
        self.device = cost.device

    @torch.no_grad()
    def path(self, start_cell, max_len=None):
        """The cells int32 [L,3] (on the device) from `start_cell` down to a seed, both included (gs_geodesic_path): each
        step takes the allowed neighbour with the smallest cost + weight, ties to the lowest move index.  L = 0 when
        the start holds INF.  `max_len` defaults to min(number of cells, cost[start] / 1000 + 2), which always suffices;
        RuntimeError when a given max_len does not.  One 4-byte read of cost[start], one of the length."""
        what = "GeodesicField.path"
        c = _cell(start_cell, self.dims, what)
        if max_len is not None and (isinstance(max_len, bool) or int(max_len) != max_len or int(max_len) < 1):
            raise ValueError(f"{what}: max_len must be a positive integer (got {max_len!r})")
        at_start = int(self.cost[c[0], c[1], c[2]].item())
        if at_start >= INF:
            return torch.zeros((0, 3), dtype=torch.int32, device=self.device)
        if max_len is None:
            max_len = min(self.cost.numel(), at_start // 1000 + 2)
        max_len = int(max_len)
        cells = torch.empty((max_len, 3), dtype=torch.int32, device=self.device)
        n = torch.empty(1, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            rc = _lib.lib().gs_geodesic_path(_lib.ptr(self.cost), _lib.ptr(self.passable), *self.dims, *c, max_len,
                                             _lib.ptr(cells), _lib.ptr(n), _lib.stream_ptr(self.device))
        _lib.check(rc, what)
        n = int(n.item())
        if n < 0:
            raise RuntimeError(f"{what}: {max_len} cells do not reach a seed from {tuple(c)} (cost {at_start})")
        return cells[:n]


def field_arguments(passable, seeds, max_cost=None, max_sweeps=65536):
    """(dims, seeds int32 [m,3] on the host, max_cost, max_sweeps) of `geodesic_field`, or ValueError.  Touches no
    device."""
    what = "geodesic_field"
    if not isinstance(passable, torch.Tensor) or passable.dtype not in (torch.uint8, torch.bool):
        raise ValueError(f"{what}: passable must be a uint8 or bool tensor "
                         f"(got {getattr(passable, 'dtype', type(passable).__name__)})")
    if passable.dim() != 3 or not all(1 <= int(n) <= MAX_CELLS for n in passable.shape):
        raise ValueError(f"{what}: passable must be [n0,n1,n2] with every size in [1, {MAX_CELLS}] "
                         f"(got {list(passable.shape)}); a 2-D map [n_u,n_v] is the lattice [1,n_u,n_v]")
    dims = tuple(int(n) for n in passable.shape)
    s = seeds.detach().cpu().numpy() if isinstance(seeds, torch.Tensor) else np.asarray(seeds)
    if s.size == 0:
        s = np.zeros((0, 3), dtype=np.int32)
    if s.ndim != 2 or s.shape[1] != 3 or not (np.issubdtype(s.dtype, np.integer) and s.dtype != np.bool_):
        raise ValueError(f"{what}: seeds must be integers [m,3] (got {s.dtype} {list(s.shape)})")
    if ((s < 0) | (s >= np.asarray(dims)[None, :])).any():
        raise ValueError(f"{what}: a seed lies outside the lattice {dims}")
    if max_cost is None:
        max_cost = MAX_COST
    if isinstance(max_cost, bool) or not isinstance(max_cost, (int, np.integer)) or not 0 <= int(max_cost) <= MAX_COST:
        raise ValueError(f"{what}: max_cost must be an integer in [0, {MAX_COST}] milli-voxels (got {max_cost!r})")
    if isinstance(max_sweeps, bool) or not isinstance(max_sweeps, (int, np.integer)) or int(max_sweeps) < 1:
        raise ValueError(f"{what}: max_sweeps must be a positive integer (got {max_sweeps!r})")
    return dims, np.ascontiguousarray(s, dtype=np.int32), int(max_cost), int(max_sweeps)


def _brick(fn_name):
    b = [ctypes.c_int(0) for _ in range(3)]
    _lib.check(getattr(_lib.lib(), fn_name)(*[ctypes.byref(v) for v in b]), fn_name)
    return tuple(v.value for v in b)


def brick():
    """The relaxation's brick (b0, b1, b2) in cells (gs_geodesic_brick)."""
    return _brick("gs_geodesic_brick")


def sweep_to_fixed_point(enqueue, changed, max_sweeps, what):
    """Brick sweeps until one lowers nothing; returns their number, that quiet one included.  `enqueue(sweep0, k)` makes
    the C call that enqueues sweeps sweep0 .. sweep0 + k - 1 and has them write `changed[:k]` (int32 [SWEEP_BATCH] on the
    device); sweeps go out in batches of SWEEP_BATCH and `changed` is read once per batch.  RuntimeError when
    `max_sweeps` sweeps do not get there."""
    sweeps = 0
    while True:
        k = min(SWEEP_BATCH, max_sweeps - sweeps)
        if k <= 0:
            raise RuntimeError(f"{what}: no fixed point after max_sweeps = {max_sweeps} sweeps")
        enqueue(sweeps, k)
        quiet = (changed[:k] == 0).cpu().tolist()                             # the batch's one read
        if True in quiet:
            return sweeps + quiet.index(True) + 1
        sweeps += k


@torch.no_grad()
def geodesic_field(passable, seeds, max_cost=None, max_sweeps=65536):
    """The cost-to-go field over `passable` (uint8 or bool [n0,n1,n2], non-zero where the robot's centre may be; on the
    GPU, or moved there) from the cells `seeds` (integers [m,3]; a blocked seed is ignored): a `GeodesicField`.  Costs
    above `max_cost` (milli-voxels, default and at most 0x3fffffff - 1732) are INF.  Sweeps are enqueued in batches of
    SWEEP_BATCH (gs_geodesic_relax) and `changed` is read once per batch until a sweep lowered nothing; RuntimeError
    when `max_sweeps` sweeps do not get there.  ValueError for bad shapes, dtypes, seeds outside the lattice or a
    max_cost out of range, before the device is touched."""
    dims, seeds, max_cost, max_sweeps = field_arguments(passable, seeds, max_cost, max_sweeps)
    L = _lib.lib()
    dev = passable.device if passable.is_cuda else torch.device("cuda", torch.cuda.current_device())
    passable = passable.to(device=dev, dtype=torch.uint8).contiguous()
    cost = torch.empty(dims, dtype=torch.int32, device=dev)
    flags = torch.empty(L.gs_geodesic_flags_bytes(*dims), dtype=torch.uint8, device=dev)
    changed = torch.empty(SWEEP_BATCH, dtype=torch.int32, device=dev)        # u32 0 / 1
    seeds_d = torch.from_numpy(seeds).to(dev)
    m = int(seeds.shape[0])
    with torch.cuda.device(dev):
        stream = _lib.stream_ptr(dev)
        _lib.check(L.gs_geodesic_init(_lib.ptr(passable), *dims, _lib.ptr(seeds_d) if m else None, m, _lib.ptr(cost),
                                      _lib.ptr(flags), stream), "geodesic_field (init)")
        sweeps = sweep_to_fixed_point(
            lambda sweep0, k: _lib.check(L.gs_geodesic_relax(_lib.ptr(passable), *dims, max_cost, _lib.ptr(cost),
                                                             _lib.ptr(flags), sweep0, k, _lib.ptr(changed), stream),
                                         "geodesic_field (relax)"),
            changed, max_sweeps, "geodesic_field")
    return GeodesicField(cost, passable, sweeps)


def snap_cell(passable, cell, radius_cells):
    """`cell` (three integers, possibly outside the lattice) if it is inside and passable, else the passable cell at the
    smallest squared lattice distance <= radius_cells^2 from it, ties to the lowest linear index, else None.  torch on
    the window of the lattice that the radius covers; one small read."""
    dims = tuple(int(n) for n in passable.shape)
    c = [int(v) for v in cell]
    inside = all(0 <= c[i] < dims[i] for i in range(3))
    if inside and int(passable[c[0], c[1], c[2]].item()) != 0:
        return c
    r = int(math.floor(radius_cells))
    if r <= 0:
        return None
    lo = [max(c[i] - r, 0) for i in range(3)]
    hi = [min(c[i] + r, dims[i] - 1) for i in range(3)]
    if any(lo[i] > hi[i] for i in range(3)):
        return None
    dev = passable.device
    ax = [torch.arange(lo[i], hi[i] + 1, dtype=torch.int64, device=dev) for i in range(3)]
    g0, g1, g2 = torch.meshgrid(*ax, indexing="ij")
    d2 = (g0 - c[0]) ** 2 + (g1 - c[1]) ** 2 + (g2 - c[2]) ** 2
    lin = (g0 * dims[1] + g1) * dims[2] + g2
    window = passable[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1] != 0
    ok = window & (d2.double() <= float(radius_cells) ** 2)
    key = torch.where(ok, d2 * (1 << 31) + lin, torch.full_like(d2, 1 << 62))    # d2 <= 3 * 1024^2, lin < 2^30
    best = int(key.min().item())
    if best >= 1 << 62:
        return None
    lin = best & ((1 << 31) - 1)
    return [lin // (dims[1] * dims[2]), lin // dims[2] % dims[1], lin % dims[2]]


def map_cell(shape, origin, res, xy, name, what):
    """The cell (u, v) = floor((xy - origin) / res) of the map point `xy` on a 2-D map of `shape`, or ValueError for a
    point that is no two finite numbers or lies outside the map."""
    try:
        x, y = (float(v) for v in xy)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: {name} must be (x, y) (got {xy!r})") from None
    if not (math.isfinite(x) and math.isfinite(y)):
        raise ValueError(f"{what}: {name} {xy!r} is not finite")
    uv = (int(math.floor((x - origin[0]) / res)), int(math.floor((y - origin[1]) / res)))
    if not (0 <= uv[0] < shape[0] and 0 <= uv[1] < shape[1]):
        raise ValueError(f"{what}: {name} {xy!r} is cell {uv}, outside the map {list(shape)}")
    return uv


@torch.no_grad()
def plan_on_map(grid, start_xy, goal_xy, allow_unknown=False, straighten=False, window=DEFAULT_WINDOW):
    """Plan on the 2-D map `grid` (the dict of `ESDF.occupancy_slice` or `load_map`: cells uint8 [n_u,n_v], origin,
    resolution) from `start_xy` to `goal_xy` (map coordinates along the two image axes).  A cell passes when it is free
    (254), with `allow_unknown` also when unknown (205); the lattice is [1,n_u,n_v]; a point's cell is
    floor((xy - origin) / resolution).  -> {"reachable", "cells": int32 [L,2] (u, v) start to goal on the device,
    "points": float64 [L,2], their centres origin + (cell + 0.5) * resolution, "length_m", "start_cell", "goal_cell",
    "sweeps"}; unreachable: L = 0 and length_m inf.  With `straighten` the dict gains `with_waypoints`' keys
    ("waypoint_index", "waypoints" int32 [K,2], "waypoint_points" float64 [K,2], "straight_length_m": the shortest route
    over the path's own cells by straight legs across passable cells, each cell tested against the `window` before it);
    without it nothing else is launched.  ValueError for a point outside the map or a bad window, before the device is
    touched."""
    what = "plan_on_map"
    window = _window(window, what)
    cells = grid["cells"]
    cells = cells if isinstance(cells, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(cells))
    if cells.dim() != 2 or cells.dtype != torch.uint8:
        raise ValueError(f"{what}: cells must be uint8 [n_u,n_v] (got {cells.dtype} {list(cells.shape)})")
    res = float(grid["resolution"])
    origin = [float(v) for v in grid["origin"]]
    if not res > 0:
        raise ValueError(f"{what}: resolution must be positive (got {res})")
    ends = [map_cell(cells.shape, origin, res, xy, name, what)
            for name, xy in (("start_xy", start_xy), ("goal_xy", goal_xy))]
    passable = cells == MAP_FREE
    if allow_unknown:
        passable = passable | (cells == MAP_UNKNOWN)
    field = geodesic_field(passable[None].contiguous(), [[0, ends[1][0], ends[1][1]]])
    path = field.path([0, ends[0][0], ends[0][1]])[:, 1:].contiguous()
    reachable = int(path.shape[0]) > 0
    length = float(field.cost[0, ends[0][0], ends[0][1]].item()) * res / 1000.0 if reachable else math.inf
    points = torch.tensor(origin, dtype=torch.float64, device=path.device)[None, :] + (path.double() + 0.5) * res
    out = {"reachable": reachable, "cells": path, "points": points, "length_m": length, "start_cell": ends[0],
           "goal_cell": ends[1], "sweeps": field.sweeps}
    if straighten:
        corner = torch.tensor(origin, dtype=torch.float64, device=path.device)[None, :]
        out = with_waypoints(out, field.passable, window, lambda c: corner + (c.double() + 0.5) * res, res, what=what)
    return out


# ---- line of sight and the shortest shortcut of a path (csrc/sight.hip) ---------------------------------------------------
def _sight_lattice(t, name, dtypes, what):
    """dims of the lattice tensor `t`, or ValueError."""
    if not isinstance(t, torch.Tensor) or t.dtype not in dtypes:
        raise ValueError(f"{what}: {name} must be a tensor of {' or '.join(str(d).replace('torch.', '') for d in dtypes)} "
                         f"(got {getattr(t, 'dtype', type(t).__name__)})")
    if t.dim() != 3 or not all(1 <= int(n) <= MAX_CELLS for n in t.shape):
        raise ValueError(f"{what}: {name} must be [n0,n1,n2] with every size in [1, {MAX_CELLS}] (got {list(t.shape)}); "
                         "a 2-D map [n_u,n_v] is the lattice [1,n_u,n_v]")
    return tuple(int(n) for n in t.shape)


def _cell_rows(cells, name, what):
    """`cells` (a tensor or anything numpy reads) as it is when an integer tensor [n,3], else as an int32 host tensor
    [n,3]; ValueError for another shape or for numbers that are no integers.  Touches no device."""
    if isinstance(cells, torch.Tensor):
        if cells.dim() != 2 or cells.shape[1] != 3 or cells.dtype not in (torch.int32, torch.int64, torch.int16, torch.uint8):
            raise ValueError(f"{what}: {name} must be integers [n,3] (got {cells.dtype} {list(cells.shape)})")
        return cells
    c = np.asarray(cells)
    if c.size == 0:
        c = np.zeros((0, 3), dtype=np.int32)
    if c.ndim != 2 or c.shape[1] != 3 or not np.issubdtype(c.dtype, np.integer):
        raise ValueError(f"{what}: {name} must be integers [n,3] (got {c.dtype} {list(c.shape)})")
    if c.size and (c.min() < -2 ** 31 or c.max() >= 2 ** 31):
        raise ValueError(f"{what}: {name} must be integers that fit 32 bits")
    return torch.from_numpy(np.ascontiguousarray(c, dtype=np.int32))


def _segments(lattice, a, b, what):
    """(the lattice on the GPU, segs int32 [n,6] beside it) for the cells `a` and `b` [n,3]."""
    a, b = _cell_rows(a, "a", what), _cell_rows(b, "b", what)
    if a.shape != b.shape:
        raise ValueError(f"{what}: a is {list(a.shape)} and b is {list(b.shape)}")
    dev = lattice.device if lattice.is_cuda else torch.device("cuda", torch.cuda.current_device())
    segs = torch.cat([a.to(device=dev, dtype=torch.int32), b.to(device=dev, dtype=torch.int32)], dim=1).contiguous()
    return lattice.to(dev), segs


@torch.no_grad()
def line_of_sight(passable, a, b):
    """bool [n] on the device: whether the cell a[i] sees the cell b[i] over `passable` (uint8 or bool [n0,n1,n2]; on the
    GPU, or moved there), i.e. both lie inside the lattice and every cell whose closed unit cube the straight segment
    between the two centres meets is passable (gs_segment_sight): a robot whose centre may be at the passable cells may go
    straight from a to b.  `a`, `b`: integers [n,3], tensors or arrays; a cell outside the lattice sees nothing.  One
    launch, nothing is read back.  ValueError for bad shapes or dtypes before the device is touched."""
    what = "line_of_sight"
    dims = _sight_lattice(passable, "passable", (torch.uint8, torch.bool), what)
    passable, segs = _segments(passable, a, b, what)
    passable = passable.to(torch.uint8).contiguous()
    n = int(segs.shape[0])
    out = torch.empty(n, dtype=torch.uint8, device=segs.device)
    with torch.cuda.device(segs.device):
        _lib.check(_lib.lib().gs_segment_sight(_lib.ptr(passable), *dims, _lib.ptr(segs), n, _lib.ptr(out),
                                               _lib.stream_ptr(segs.device)), what)
    return out != 0


@torch.no_grad()
def segment_min(field, a, b):
    """(value int32 [n], cell int32 [n]) on the device: the smallest value of `field` (int32 [n0,n1,n2]; on the GPU, or
    moved there) over the cells the straight segment from a[i] to b[i] meets (`line_of_sight`'s cells) and the lowest
    linear index that holds it (gs_segment_min); INT32_MIN and -1 when an end lies outside the lattice.  With ESDF.d2 as
    the field it is the squared clearance of a straight leg.  One launch, nothing is read back."""
    what = "segment_min"
    dims = _sight_lattice(field, "field", (torch.int32,), what)
    field, segs = _segments(field, a, b, what)
    field = field.contiguous()
    n = int(segs.shape[0])
    value = torch.empty(n, dtype=torch.int32, device=segs.device)
    cell = torch.empty(n, dtype=torch.int32, device=segs.device)
    with torch.cuda.device(segs.device):
        _lib.check(_lib.lib().gs_segment_min(_lib.ptr(field), *dims, _lib.ptr(segs), n, _lib.ptr(value), _lib.ptr(cell),
                                             _lib.stream_ptr(segs.device)), what)
    return value, cell


def _window(window, what):
    if isinstance(window, bool) or not isinstance(window, (int, np.integer)) or int(window) < 1:
        raise ValueError(f"{what}: window must be a positive integer (got {window!r})")
    return int(window)


def straighten_arguments(passable, cells, window=DEFAULT_WINDOW, what="straighten"):
    """(dims, cells as `_cell_rows` gives them, window) of `straighten`, or ValueError.  Touches no device."""
    dims = _sight_lattice(passable, "passable", (torch.uint8, torch.bool), what)
    cells = _cell_rows(cells, "cells", what)
    if int(cells.shape[0]) < 1:
        raise ValueError(f"{what}: a path has at least one cell (got {list(cells.shape)})")
    return dims, cells, _window(window, what)


@torch.no_grad()
def straighten(passable, cells, window=DEFAULT_WINDOW):
    """The shortest route from the first to the last of the path's `cells` (integers [L,3], L >= 1) that stops only at
    cells of the path and whose every straight leg the robot may take (`line_of_sight` over `passable`): each cell is
    tested against the `window` cells before it (gs_path_sight; the window is cut to L - 1) and a dynamic programme
    picks the stops (gs_path_shortcut; equal lengths go to the earlier stop).  -> {"index": int32 [K], the kept cells'
    positions in the path, ascending, 0 and L - 1 always among them, "cells": int32 [K,3], both on the device, "length":
    the route's length in milli-voxels (a leg is floor(1000 * its Euclidean length in cells)), "window": the window
    used}.  A lattice path's own moves see, so the result is never longer than the path and `window` = 1 returns the path.
    A path of more than PATH_MAX_CELLS = 16384 cells is straightened in consecutive pieces of that many cells that share
    an end cell, which is kept: a limit, since no leg spans two pieces.  One read per piece: K and the length together.
    ValueError before the device is touched; RuntimeError when the last cell cannot be reached, that is when some cell
    sees none of the `window` before it (a path through blocked cells)."""
    what = "straighten"
    dims, cells, window = straighten_arguments(passable, cells, window, what)
    L_all = int(cells.shape[0])
    L = _lib.lib()
    dev = passable.device if passable.is_cuda else torch.device("cuda", torch.cuda.current_device())
    passable = passable.to(device=dev, dtype=torch.uint8).contiguous()
    cells = cells.to(device=dev, dtype=torch.int32).contiguous()
    kept, length, used = [], 0, 1
    with torch.cuda.device(dev):
        stream = _lib.stream_ptr(dev)
        for first in range(0, max(L_all - 1, 1), PATH_MAX_CELLS - 1):
            piece = cells[first:first + PATH_MAX_CELLS]
            n = int(piece.shape[0])
            w = max(min(window, n - 1), 1)
            used = max(used, w)
            sight = torch.empty((n, (w + 63) // 64), dtype=torch.int64, device=dev)             # u64 words
            index = torch.empty(n, dtype=torch.int32, device=dev)
            tail = torch.empty(2, dtype=torch.int32, device=dev)                                 # n_out, length
            _lib.check(L.gs_path_sight(_lib.ptr(passable), *dims, _lib.ptr(piece), n, w, _lib.ptr(sight), stream),
                       f"{what} (sight)")
            _lib.check(L.gs_path_shortcut(_lib.ptr(sight), _lib.ptr(piece), n, w, _lib.ptr(index), _lib.ptr(tail[0:]),
                                          _lib.ptr(tail[1:]), stream), f"{what} (shortcut)")
            k, piece_length = tail.cpu().tolist()                                                # the piece's one read
            if k < 0:
                raise RuntimeError(f"{what}: cell {first + n - 1} of the path cannot be reached from cell {first} with a "
                                   f"window of {w}: some cell in between sees none of the {w} before it")
            kept.append(index[0 if first == 0 else 1:k] + first)
            length += piece_length
    index = kept[0] if len(kept) == 1 else torch.cat(kept)
    return {"index": index, "cells": cells[index.long()], "length": length, "window": used}


@torch.no_grad()
def with_waypoints(route, passable, window, to_points, metres_per_cell, d2=None, dist=None, what="straighten"):
    """`route` (the dict of `ESDF.plan` or `plan_on_map`; not changed) with the keys of its straightened form added:
    "waypoint_index" int32 [K] and "waypoints", the kept cells (as `cells` has them: [K,3], or [K,2] on a map), on the
    device, "waypoint_points" float64 = to_points(waypoints), "straight_length_m" = the straightened length *
    metres_per_cell / 1000, and with `d2` and `dist` (the ESDF's) "straight_min_clearance_m": `dist` at the cell that
    `segment_min` reports for `d2` over the kept legs, the smallest of them, ties to the lowest linear index.  An
    unreachable route gets empty waypoints, inf and nan.  Reads: `straighten`'s, and one for the clearance."""
    cells = route["cells"]
    out = dict(route)
    if not isinstance(cells, torch.Tensor) or cells.dim() != 2 or cells.shape[1] not in (2, 3):
        raise ValueError(f"{what}: a route's cells are [L,3] or [L,2] (got {getattr(cells, 'shape', cells)!r})")
    flat = int(cells.shape[1]) == 2
    window = _window(window, what)
    if int(cells.shape[0]) == 0:
        out.update(waypoint_index=torch.zeros(0, dtype=torch.int32, device=cells.device), waypoints=cells[:0],
                   waypoint_points=to_points(cells[:0]), straight_length_m=math.inf)
        if d2 is not None:
            out["straight_min_clearance_m"] = math.nan
        return out
    cells3 = torch.cat([torch.zeros_like(cells[:, :1]), cells], dim=1) if flat else cells
    res = straighten(passable, cells3, window)
    way = res["cells"][:, 1:].contiguous() if flat else res["cells"]
    out.update(waypoint_index=res["index"], waypoints=way, waypoint_points=to_points(way),
               straight_length_m=res["length"] * metres_per_cell / 1000.0)
    if d2 is not None:
        legs = res["cells"]
        value, cell = segment_min(d2, legs[:-1] if len(legs) > 1 else legs, legs[1:] if len(legs) > 1 else legs)
        worst = int((value.long() * (1 << 32) + cell.long()).min().item()) & 0xffffffff          # one read
        out["straight_min_clearance_m"] = float(dist.reshape(-1)[worst].item())
    return out


STRAIGHT_REPORT_ORDER = ("reachable", "length_m", "min_clearance_m", "n_points", "lattice_length_m", "n_lattice_points")
_STRAIGHT_HEADER = "Straightened collision-free path"


def straight_path_text(result):
    """The text of map/path_straight.txt for the dict of `ESDF.plan(..., straighten=True)`: `path_text`'s layout with a
    header of its own -- two header lines, `name<TAB>repr(value)` for reachable, length_m (the straightened length),
    min_clearance_m (along the straight legs), n_points, lattice_length_m and n_lattice_points (the lattice route's), then
    one `x y z` line per waypoint with repr(): reading the file gives back the numbers bit for bit."""
    pts = result["waypoint_points"]
    pts = pts.detach().cpu().numpy() if isinstance(pts, torch.Tensor) else np.asarray(pts)
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    head = {"reachable": bool(result["reachable"]), "length_m": float(result["straight_length_m"]),
            "min_clearance_m": float(result["straight_min_clearance_m"]), "n_points": int(pts.shape[0]),
            "lattice_length_m": float(result["length_m"]), "n_lattice_points": int(result["cells"].shape[0])}
    lines = [_STRAIGHT_HEADER + " through the fused TSDF volume's distance field, start to goal: the waypoints [m], cells "
             "of the lattice route of map/path.txt joined by straight legs that keep the robot's radius from every surface",
             "(length_m: the legs' length; min_clearance_m: the smallest distance to a surface along them; "
             "lattice_length_m, n_lattice_points: the lattice route's; inf and nan when the goal cannot be reached; then per "
             "waypoint: x y z)"]
    lines += [f"{k}\t{head[k]!r}" for k in STRAIGHT_REPORT_ORDER]
    lines += [f"{float(p[0])!r} {float(p[1])!r} {float(p[2])!r}" for p in pts]
    return "\n".join(lines) + "\n"


def parse_straight_path(text):
    """straight_path_text's inverse: (the dict of STRAIGHT_REPORT_ORDER, waypoints float64 [n,3])."""
    lines = text.splitlines()
    if len(lines) < 2 + len(STRAIGHT_REPORT_ORDER) or not lines[0].startswith(_STRAIGHT_HEADER):
        raise ValueError("not a map/path_straight.txt")
    result = {}
    for key, line in zip(STRAIGHT_REPORT_ORDER, lines[2:]):
        name, _, value = line.partition("\t")
        if name != key:
            raise ValueError(f"path_straight.txt: expected {key}, found {name}")
        if key == "reachable":
            if value not in ("True", "False"):
                raise ValueError(f"path_straight.txt: reachable is {value!r}")
            result[key] = value == "True"
        else:
            result[key] = int(value) if key in ("n_points", "n_lattice_points") else float(value)
    rows = [[float(v) for v in line.split(" ")] for line in lines[2 + len(STRAIGHT_REPORT_ORDER):]]
    if len(rows) != result["n_points"] or any(len(r) != 3 for r in rows):
        raise ValueError("path_straight.txt: the waypoints do not match n_points")
    return result, np.array(rows, dtype=np.float64).reshape(-1, 3)


def straighten_config(value, what="tsdf.esdf.plan.straighten"):
    """None when the config value (absent, a bool, or {enable, window}) switches straightening off, else the window;
    ValueError for anything else."""
    if value is None or value is False:
        return None
    if value is True:
        return DEFAULT_WINDOW
    if not isinstance(value, dict) or set(value) - {"enable", "window"} or not isinstance(value.get("enable", True), bool):
        raise ValueError(f"{what} must be a bool or {{enable, window}} (got {value!r})")
    window = _window(value.get("window", DEFAULT_WINDOW), what)
    return window if value.get("enable", True) else None


PATH_REPORT_ORDER = ("reachable", "length_m", "min_clearance_m", "n_points")


def path_text(result):
    """The text of map/path.txt for `ESDF.plan`'s dict: two header lines, `name<TAB>repr(value)` for reachable,
    length_m, min_clearance_m and n_points, then one `x y z` line per point with repr(): reading the file gives back
    the numbers bit for bit."""
    pts = result["points"]
    pts = pts.detach().cpu().numpy() if isinstance(pts, torch.Tensor) else np.asarray(pts)
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    head = {"reachable": bool(result["reachable"]), "length_m": float(result["length_m"]),
            "min_clearance_m": float(result["min_clearance_m"]), "n_points": int(pts.shape[0])}
    lines = ["Collision-free path through the fused TSDF volume's distance field, start to goal: the centres [m] of the "
             "lattice cells of the shortest route that keeps the robot's radius from every surface",
             "(length_m: its length; min_clearance_m: the smallest distance to a surface along it; inf and nan when the "
             "goal cannot be reached; then per point: x y z)"]
    lines += [f"{k}\t{head[k]!r}" for k in PATH_REPORT_ORDER]
    lines += [f"{float(p[0])!r} {float(p[1])!r} {float(p[2])!r}" for p in pts]
    return "\n".join(lines) + "\n"


def parse_path(text):
    """path_text's inverse: ({"reachable", "length_m", "min_clearance_m", "n_points"}, points float64 [n,3])."""
    lines = text.splitlines()
    if len(lines) < 2 + len(PATH_REPORT_ORDER) or not lines[0].startswith("Collision-free path through"):
        raise ValueError("not a map/path.txt")
    result = {}
    for key, line in zip(PATH_REPORT_ORDER, lines[2:]):
        name, value = line.split("\t")
        if name != key:
            raise ValueError(f"path.txt: expected {key}, found {name}")
        if key == "reachable":
            if value not in ("True", "False"):
                raise ValueError(f"path.txt: reachable is {value!r}")
            result[key] = value == "True"
        else:
            result[key] = int(value) if key == "n_points" else float(value)
    rows = [[float(v) for v in line.split(" ")] for line in lines[2 + len(PATH_REPORT_ORDER):]]
    if len(rows) != result["n_points"] or any(len(r) != 3 for r in rows):
        raise ValueError("path.txt: the points do not match n_points")
    return result, np.array(rows, dtype=np.float64).reshape(-1, 3)
