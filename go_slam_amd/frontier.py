"""Frontiers of a state lattice: the free cells that border never-observed space, grouped into clusters a planner can
choose between, each with its size, area, centroid, box and cheapest cell (csrc/frontier.hip).

`frontier_clusters` marks the frontier cells of a lattice of states (0 unknown, 1 free, 2 solid), labels their
26-connected components by relaxing, brick by brick on the GPU, every cell's label to the smallest of its neighbours'
until nothing falls, and accumulates one table row per component.  Everything is integer and the labels are the unique
fixed point of their relaxation, so they equal a serial flood fill bit for bit (tests/frontier_restatement.py;
include/goslam_hip.h, gs_frontier_*).  `ESDF.frontiers` / `explore` (tsdf.py) put a fused volume's
distance field under it and price every cluster with one `plan.geodesic_field`, `frontiers_on_map` does the same over a
2-D occupancy map, and `frontiers_text` / `parse_frontiers` are the run's map/frontiers.txt.
"""
import math

import numpy as np
import torch

from . import _lib
from . import plan as _plan

INF = _plan.INF                        # GS_GEO_INF
MAX_CELLS = _plan.MAX_CELLS            # per axis
SWEEP_BATCH = _plan.SWEEP_BATCH        # sweeps enqueued per host read of `changed`
ORDERS = ("nearest", "largest")


class FrontierClusters:
    """The frontier of a lattice at its fixed point.  `.frontier` uint8 [n0,n1,n2] (1 on a frontier cell), `.label` int32
    [n0,n1,n2] (-1 off the frontier, else the smallest linear index of the cell's cluster), `.counts` int64 [4] (unknown,
    free, solid and frontier cells; on the device), the table's columns, one row per cluster by ascending root, on the
    device -- `.root`, `.size`, `.faces`, `.best_cost`, `.best_cell` int32 [K], `.sum` int64 [K,3], `.bbox` int32 [K,6]
    (mins, then maxes) -- `.n_clusters` = K, `.dims`, and `.sweeps`, the number of brick sweeps that were needed (the
    last of them lowered nothing; it may differ between runs, the labels do not)."""

    def __init__(self, frontier, label, counts, table, sweeps):
        self.frontier, self.label, self.counts, self.sweeps = frontier, label, counts, int(sweeps)
        self.root, self.size, self.faces = table["root"], table["size"], table["faces"]
        self.sum, self.bbox = table["sum"], table["bbox"]
        self.best_cost, self.best_cell = table["best_cost"], table["best_cell"]
        self.n_clusters = int(self.root.shape[0])
        self.dims = tuple(int(n) for n in label.shape)
        self.device = label.device

    def centroid_cells(self):
        """float64 [K,3]: the mean coordinates of every cluster's cells, in cells."""
        return self.sum.double() / self.size.double()[:, None]


def cluster_arguments(state, open=None, cost=None, max_sweeps=65536):
    """(dims, max_sweeps) of `frontier_clusters`, or ValueError.  Touches no device."""
    what = "frontier_clusters"
    if not isinstance(state, torch.Tensor) or state.dtype != torch.uint8:
        raise ValueError(f"{what}: state must be a uint8 tensor (got {getattr(state, 'dtype', type(state).__name__)})")
    if state.dim() != 3 or not all(1 <= int(n) <= MAX_CELLS for n in state.shape):
        raise ValueError(f"{what}: state must be [n0,n1,n2] with every size in [1, {MAX_CELLS}] "
                         f"(got {list(state.shape)}); a 2-D map [n_u,n_v] is the lattice [1,n_u,n_v]")
    dims = tuple(int(n) for n in state.shape)
    if open is not None:
        if not isinstance(open, torch.Tensor) or open.dtype not in (torch.uint8, torch.bool):
            raise ValueError(f"{what}: open must be a uint8 or bool tensor or None "
                             f"(got {getattr(open, 'dtype', type(open).__name__)})")
        if tuple(open.shape) != dims:
            raise ValueError(f"{what}: open is {list(open.shape)}, state is {list(dims)}")
    if cost is not None:
        if not isinstance(cost, torch.Tensor) or cost.dtype != torch.int32:
            raise ValueError(f"{what}: cost must be an int32 tensor or None "
                             f"(got {getattr(cost, 'dtype', type(cost).__name__)})")
        if tuple(cost.shape) != dims:
            raise ValueError(f"{what}: cost is {list(cost.shape)}, state is {list(dims)}")
    if isinstance(max_sweeps, bool) or not isinstance(max_sweeps, (int, np.integer)) or int(max_sweeps) < 1:
        raise ValueError(f"{what}: max_sweeps must be a positive integer (got {max_sweeps!r})")
    return dims, int(max_sweeps)


def brick():
    """The relaxation's brick (b0, b1, b2) in cells (gs_frontier_brick)."""
    return _plan._brick("gs_frontier_brick")


@torch.no_grad()
def frontier_clusters(state, open=None, cost=None, max_sweeps=65536):
    """The frontier cells of `state` (uint8 [n0,n1,n2]: 0 unknown, 1 free, 2 solid; on the GPU, or moved there), their
    26-connected clusters and the cluster table: a `FrontierClusters`.  A frontier cell is free, lies in `open` (uint8
    or bool, same shape; None: every free cell) and has a face neighbour inside the lattice that is unknown.  `cost`
    (int32, same shape: a `GeodesicField.cost`; None: INF everywhere) prices the clusters: `best_cost` / `best_cell` are
    the cheapest cell of each, ties to the lowest index.  Sweeps are enqueued in batches of SWEEP_BATCH
    (gs_frontier_relax) and `changed` is read once per batch until a sweep lowered nothing; RuntimeError when `max_sweeps`
    sweeps do not get there.  Host reads per call: one per batch of sweeps (SWEEP_BATCH words) and one of the number of
    clusters (4 bytes), which sizes the table; nothing else leaves the device.  ValueError for bad shapes or dtypes,
    before the device is touched."""
    dims, max_sweeps = cluster_arguments(state, open, cost, max_sweeps)
    L = _lib.lib()
    dev = state.device if state.is_cuda else torch.device("cuda", torch.cuda.current_device())
    state = state.to(dev).contiguous()
    open = None if open is None else open.to(device=dev, dtype=torch.uint8).contiguous()
    cost = None if cost is None else cost.to(dev).contiguous()
    frontier = torch.empty(dims, dtype=torch.uint8, device=dev)
    label = torch.empty(dims, dtype=torch.int32, device=dev)
    counts = torch.empty(4, dtype=torch.int32, device=dev)                    # u32, each at most 2^30
    flags = torch.empty(L.gs_frontier_flags_bytes(*dims), dtype=torch.uint8, device=dev)
    changed = torch.empty(SWEEP_BATCH, dtype=torch.int32, device=dev)        # u32 0 / 1
    ws_bytes = L.gs_frontier_workspace_bytes(*dims)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    n_roots = torch.empty(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        stream = _lib.stream_ptr(dev)
        _lib.check(L.gs_frontier_mark(_lib.ptr(state), _lib.ptr(open), *dims, _lib.ptr(frontier), _lib.ptr(label),
                                      _lib.ptr(counts), _lib.ptr(flags), stream), "frontier_clusters (mark)")
        sweeps = _plan.sweep_to_fixed_point(
            lambda sweep0, k: _lib.check(L.gs_frontier_relax(*dims, _lib.ptr(label), _lib.ptr(flags), sweep0, k,
                                                             _lib.ptr(changed), stream), "frontier_clusters (relax)"),
            changed, max_sweeps, "frontier_clusters")
        _lib.check(L.gs_frontier_roots(_lib.ptr(label), *dims, _lib.ptr(ws), ws_bytes, _lib.ptr(n_roots), stream),
                   "frontier_clusters (roots)")
        K = int(n_roots.item())                                               # the read that sizes the table
        table = {"root": torch.empty(K, dtype=torch.int32, device=dev), "size": torch.empty(K, dtype=torch.int32, device=dev),
                 "faces": torch.empty(K, dtype=torch.int32, device=dev),
                 "sum": torch.empty((K, 3), dtype=torch.int64, device=dev),
                 "bbox": torch.empty((K, 6), dtype=torch.int32, device=dev)}
        best = torch.empty((K, 2), dtype=torch.int32, device=dev)             # (best_cell, best_cost): one u64 key per row
        if K > 0:
            _lib.check(L.gs_frontier_table(_lib.ptr(state), _lib.ptr(label), _lib.ptr(cost), *dims, _lib.ptr(ws), ws_bytes,
                                           K, K, _lib.ptr(table["root"]), _lib.ptr(table["size"]),
                                           _lib.ptr(table["faces"]), _lib.ptr(table["sum"]), _lib.ptr(table["bbox"]),
                                           _lib.ptr(best), stream), "frontier_clusters (table)")
    table["best_cell"], table["best_cost"] = best[:, 0], best[:, 1]
    return FrontierClusters(frontier, label, counts.long(), table, sweeps)


def _min_cells(min_cells, what):
    if isinstance(min_cells, bool) or not isinstance(min_cells, (int, np.integer)) or int(min_cells) < 1:
        raise ValueError(f"{what}: min_cells must be a positive integer (got {min_cells!r})")
    return int(min_cells)


@torch.no_grad()
def frontiers_on_map(grid, start_xy=None, min_cells=1):
    """The frontiers of the 2-D map `grid` (the dict of `ESDF.occupancy_slice` or `load_map`: cells uint8 [n_u,n_v],
    origin, resolution): a `FrontierClusters` over the lattice [1,n_u,n_v] with a cell free when it is 254, unknown when
    205, solid otherwise, and `open` = free.  With `start_xy` (map coordinates; its cell is floor((xy - origin) /
    resolution), as in `plan_on_map`) a `plan.geodesic_field` over the free cells seeded there prices the clusters.
    Extras: `.centroid` float64 [K,2] = origin + (centroid_cells[:, 1:] + 0.5) * resolution, `.length_m` float64 [K] =
    faces * resolution (in a plane a frontier is a line), `.cost_m` float64 [K] = best_cost * resolution / 1000, inf
    where INF, `.keep` bool [K] = size >= min_cells, `.start_cell` (u, v) or None, `.field` (the GeodesicField or None).
    ValueError for a point outside the map, before the device is touched."""
    what = "frontiers_on_map"
    cells = grid["cells"]
    cells = cells if isinstance(cells, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(cells))
    if cells.dim() != 2 or cells.dtype != torch.uint8:
        raise ValueError(f"{what}: cells must be uint8 [n_u,n_v] (got {cells.dtype} {list(cells.shape)})")
    res = float(grid["resolution"])
    origin = [float(v) for v in grid["origin"]]
    if not res > 0:
        raise ValueError(f"{what}: resolution must be positive (got {res})")
    min_cells = _min_cells(min_cells, what)
    start = None if start_xy is None else _plan.map_cell(cells.shape, origin, res, start_xy, "start_xy", what)
    free = cells == _plan.MAP_FREE
    state = torch.where(free, 1, torch.where(cells == _plan.MAP_UNKNOWN, 0, 2)).to(torch.uint8)[None].contiguous()
    field = None
    if start is not None:
        field = _plan.geodesic_field(free[None].contiguous(), [[0, start[0], start[1]]])
    out = frontier_clusters(state, free[None].contiguous(), None if field is None else field.cost)
    out.centroid = (torch.tensor(origin, dtype=torch.float64, device=out.device)[None, :]
                    + (out.centroid_cells()[:, 1:] + 0.5) * res)
    out.length_m = out.faces.double() * res
    out.cost_m = torch.where(out.best_cost >= INF, math.inf, out.best_cost.double() * res / 1000.0)
    out.keep = out.size >= min_cells
    out.start_cell, out.field = start, field
    return out


def choose(best_cost, faces, root, keep, order="nearest"):
    """The row `ESDF.explore` goes to, or None: among the kept rows with best_cost < INF, "nearest" takes the smallest
    best_cost, ties to the lowest root; "largest" the largest faces, then the smallest best_cost, then the lowest root.
    Host lists or arrays."""
    if order not in ORDERS:
        raise ValueError(f"explore: order must be one of {ORDERS} (got {order!r})")
    rows = [i for i in range(len(root)) if keep[i] and best_cost[i] < INF]
    if not rows:
        return None
    if order == "nearest":
        return min(rows, key=lambda i: (int(best_cost[i]), int(root[i])))
    return min(rows, key=lambda i: (-int(faces[i]), int(best_cost[i]), int(root[i])))


SUMMARY_ORDER = ("n_unknown", "n_free", "n_solid", "n_frontier", "unknown_fraction", "n_clusters", "n_kept",
                 "n_reachable", "cluster")
CLUSTER_COLUMNS = ("id", "root", "size", "faces", "area_m2", "centroid_x", "centroid_y", "centroid_z", "cost_m")
_INT_COLUMNS = ("id", "root", "size", "faces")
_HEADER = "Frontiers of the fused TSDF volume"


def summary(clusters, cluster=None):
    """The dict `frontiers_text` writes, from the `FrontierClusters` of `ESDF.frontiers` (with its world-space extras)
    and the id of the chosen cluster or None: the SUMMARY_ORDER keys and "clusters", {column: array [n_kept]} of the kept
    rows in CLUSTER_COLUMNS order.  One read of the counts and the table."""
    counts = [int(v) for v in clusters.counts.cpu().tolist()]
    keep = clusters.keep.cpu().numpy().astype(bool)
    cost_m = clusters.cost_m.cpu().numpy()
    centroid = clusters.centroid.cpu().numpy().reshape(-1, 3)
    ids = np.nonzero(keep)[0]
    total = sum(counts[:3])
    table = {"id": ids.astype(np.int64), "root": clusters.root.cpu().numpy()[ids].astype(np.int64),
             "size": clusters.size.cpu().numpy()[ids].astype(np.int64),
             "faces": clusters.faces.cpu().numpy()[ids].astype(np.int64),
             "area_m2": clusters.area_m2.cpu().numpy()[ids].astype(np.float64),
             "centroid_x": centroid[ids, 0], "centroid_y": centroid[ids, 1], "centroid_z": centroid[ids, 2],
             "cost_m": cost_m[ids].astype(np.float64)}
    return {"n_unknown": counts[0], "n_free": counts[1], "n_solid": counts[2], "n_frontier": counts[3],
            "unknown_fraction": counts[0] / total if total else 0.0, "n_clusters": int(clusters.n_clusters),
            "n_kept": int(keep.sum()), "n_reachable": int((keep & np.isfinite(cost_m)).sum()),
            "cluster": None if cluster is None else int(cluster), "clusters": table}


def frontiers_text(result):
    """The text of map/frontiers.txt for `summary`'s dict: two header lines, `name<TAB>repr(value)` for the SUMMARY_ORDER
    keys, then one line per kept cluster with the CLUSTER_COLUMNS values written with repr(): reading the file gives back
    the numbers bit for bit."""
    table = result["clusters"]
    n = len(table["id"])
    lines = [_HEADER + "'s distance field: the free cells that border never-observed space, in 26-connected clusters",
             "(unknown_fraction: unknown cells / all cells; n_kept: clusters of at least min_cells cells; n_reachable: "
             "kept clusters a route leads to; cluster: the one chosen, or None; then per kept cluster: "
             + " ".join(CLUSTER_COLUMNS) + "; cost_m inf where no route leads)"]
    for k in SUMMARY_ORDER:
        v = result[k]
        v = None if v is None else (float(v) if k == "unknown_fraction" else int(v))
        lines.append(f"{k}\t{v!r}")
    for i in range(n):
        lines.append(" ".join(repr(int(table[c][i])) if c in _INT_COLUMNS else repr(float(table[c][i]))
                              for c in CLUSTER_COLUMNS))
    return "\n".join(lines) + "\n"


def parse_frontiers(text):
    """frontiers_text's inverse: the SUMMARY_ORDER keys and "clusters", {column: int64 or float64 array [n_kept]}."""
    lines = text.splitlines()
    if len(lines) < 2 + len(SUMMARY_ORDER) or not lines[0].startswith(_HEADER):
        raise ValueError("not a map/frontiers.txt")
    result = {}
    for key, line in zip(SUMMARY_ORDER, lines[2:]):
        name, value = line.split("\t")
        if name != key:
            raise ValueError(f"frontiers.txt: expected {key}, found {name}")
        if key == "unknown_fraction":
            result[key] = float(value)
        else:
            result[key] = None if (key == "cluster" and value == "None") else int(value)
    rows = [line.split(" ") for line in lines[2 + len(SUMMARY_ORDER):]]
    if len(rows) != result["n_kept"] or any(len(r) != len(CLUSTER_COLUMNS) for r in rows):
        raise ValueError("frontiers.txt: the rows do not match n_kept")
    result["clusters"] = {c: np.array([int(r[j]) if c in _INT_COLUMNS else float(r[j]) for r in rows],
                                      dtype=np.int64 if c in _INT_COLUMNS else np.float64).reshape(len(rows))
                          for j, c in enumerate(CLUSTER_COLUMNS)}
    return result
