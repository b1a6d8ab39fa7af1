"""View gain: how much never-observed space a camera would see from a candidate pose (csrc/view_gain.hip).

`view_gain` casts one set of integer ray directions from every candidate cell of a state lattice (0 unknown, 1 free, else
solid) and counts, per view, the distinct unknown, free and solid cells the rays cross before something solid stops them:
one workgroup per view on the GPU, the visited set one bit per cell in LDS.  The walk and the counts are integer and a
set has no order, so they equal the serial restatement bit for bit (tests/view_gain_restatement.py; include/goslam_hip.h,
gs_view_gain).  `ray_directions` makes a pinhole camera's rays, `view_box` the box around the origin
that clips none of them, `ESDF.view_candidates` / `next_view` (tsdf.py) put a fused volume's distance field and one
`plan.geodesic_field` under it, `next_view_on_map` a 2-D occupancy map, and `next_view_text` / `parse_next_view` are the
run's map/next_view.txt.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from . import plan as _plan

INF = _plan.INF                        # GS_GEO_INF
MAX_CELLS = _plan.MAX_CELLS            # per axis
MAX_DIR = 32767                        # GS_VIEW_MAX_DIR
MAX_BOX_CELLS = 1 << 20                # GS_VIEW_MAX_BOX_CELLS
MAX_RAYS = 65536
MAX_RANGE = 1771                       # cells: the largest r with r^2 <= 3 * 1023^2
CAMERA_KEYS = ("hfov_deg", "vfov_deg", "n_u", "n_v", "range_m", "pitch_deg")


def _int(v, lo, hi, name, what):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
        raise ValueError(f"{what}: {name} must be an integer in [{lo}, {hi}] (got {v!r})")
    return int(v)


def ray_directions(hfov_deg, vfov_deg, n_u, n_v, yaw, pitch=0.0, up_axis=2):
    """int32 [n_u * n_v, 3] (numpy, row v * n_u + u): the pixel-centre rays of a pinhole image of n_u x n_v pixels over
    hfov_deg x vfov_deg.  In the camera frame a ray is (tan(hfov/2) x, tan(vfov/2) y, 1) with x, y the centres of an n_u x
    n_v grid over [-1, 1]; it is pitched up by `pitch`, then turned by `yaw` about `up_axis` (radians): yaw 0 looks along
    the lower of the two other axes, positive yaw turns toward the higher one, and the image's x grows toward the higher
    one too.  Each ray is scaled so that its largest component is GS_VIEW_MAX_DIR and rounded to nearest.  Host float64."""
    what = "ray_directions"
    hfov, vfov, yaw, pitch = float(hfov_deg), float(vfov_deg), float(yaw), float(pitch)
    if not (0 < hfov < 180 and 0 < vfov < 180):
        raise ValueError(f"{what}: the fields of view must lie in (0, 180) degrees (got {hfov_deg!r}, {vfov_deg!r})")
    if not (math.isfinite(yaw) and math.isfinite(pitch)):
        raise ValueError(f"{what}: yaw and pitch must be finite (got {yaw!r}, {pitch!r})")
    n_u, n_v = _int(n_u, 1, MAX_RAYS, "n_u", what), _int(n_v, 1, MAX_RAYS, "n_v", what)
    if n_u * n_v > MAX_RAYS:
        raise ValueError(f"{what}: {n_u} x {n_v} rays, at most {MAX_RAYS}")
    up = _int(up_axis, 0, 2, "up_axis", what)
    fwd, left = [a for a in range(3) if a != up]
    x = (2.0 * np.arange(n_u, dtype=np.float64) + 1.0) / n_u - 1.0
    y = (2.0 * np.arange(n_v, dtype=np.float64) + 1.0) / n_v - 1.0
    vl = np.tile(math.tan(math.radians(hfov) / 2.0) * x, n_v)
    vu = np.repeat(math.tan(math.radians(vfov) / 2.0) * y, n_u)
    vf = np.ones_like(vl)
    vf, vu = vf * math.cos(pitch) - vu * math.sin(pitch), vf * math.sin(pitch) + vu * math.cos(pitch)
    vf, vl = vf * math.cos(yaw) - vl * math.sin(yaw), vf * math.sin(yaw) + vl * math.cos(yaw)
    d = np.zeros((n_u * n_v, 3), dtype=np.float64)
    d[:, fwd], d[:, left], d[:, up] = vf, vl, vu
    d *= MAX_DIR / np.abs(d).max(axis=1, keepdims=True)
    return np.rint(d).astype(np.int32)


def _isqrt(q):
    """floor(sqrt(q)) of non-negative int64 values below 2^62, exactly."""
    s = np.floor(np.sqrt(q.astype(np.float64))).astype(np.int64)
    s -= (s * s > q)
    s += ((s + 1) * (s + 1) <= q)
    return s


def _dirs(dirs, what):
    """`dirs` as a contiguous int32 [R,3] numpy array with every component in range, or ValueError."""
    d = dirs.detach().cpu().numpy() if isinstance(dirs, torch.Tensor) else np.asarray(dirs)
    if d.ndim != 2 or d.shape[1] != 3 or not (np.issubdtype(d.dtype, np.integer) and d.dtype != np.bool_):
        raise ValueError(f"{what}: dirs must be integers [R,3] (got {d.dtype} {list(d.shape)})")
    if not 1 <= d.shape[0] <= MAX_RAYS:
        raise ValueError(f"{what}: {d.shape[0]} rays, 1 to {MAX_RAYS} are allowed")
    if (np.abs(d.astype(np.int64)) > MAX_DIR).any():
        raise ValueError(f"{what}: a direction has a component outside [-{MAX_DIR}, {MAX_DIR}]")
    return np.ascontiguousarray(d, dtype=np.int32)


def view_box(dirs, range_cells):
    """The box (lo0, lo1, lo2, hi0, hi1, hi2) of offsets from the origin that clips no ray of `dirs` within `range_cells`:
    per axis the reach on the side of sign(d_a) is floor((range_cells + 1) * |d_a| / |d| + 1), maximised over the rays,
    and 0 on the other side.  (A visited cell c holds a point p of the ray with |p - c| <= 1/2 on every axis and has |c| <=
    range, so |p| <= range + sqrt(3)/2 and |c_a| <= |p| |d_a| / |d| + 1/2.)  Exact integers on the host."""
    what = "view_box"
    d = _dirs(dirs, what).astype(np.int64)
    r = _int(range_cells, 1, MAX_RANGE, "range_cells", what)
    n2 = (d * d).sum(axis=1)
    d = d[n2 > 0]
    lo, hi = [0, 0, 0], [0, 0, 0]
    if len(d):
        n2 = n2[n2 > 0]
        reach = _isqrt(((r + 1) * np.abs(d)) ** 2 // n2[:, None]) + 1          # floor(x / sqrt(D)) = isqrt(x^2 // D)
        for a in range(3):
            if (d[:, a] > 0).any():
                hi[a] = int(reach[d[:, a] > 0, a].max())
            if (d[:, a] < 0).any():
                lo[a] = -int(reach[d[:, a] < 0, a].max())
    return tuple(lo + hi)


def _box_cells(box):
    return (box[3] - box[0] + 1) * (box[4] - box[1] + 1) * (box[5] - box[2] + 1)


def gain_arguments(state, origins, dirs, range_cells, max_unknown=0, box=None):
    """(dims, origins, dirs int32 [R,3] on the host, range_cells, max_unknown, box) of `view_gain`, or ValueError.  Touches
    no device.  `origins` comes back as given when it is a tensor, else as an int32 numpy array."""
    what = "view_gain"
    if not isinstance(state, torch.Tensor) or state.dtype != torch.uint8:
        raise ValueError(f"{what}: state must be a uint8 tensor (got {getattr(state, 'dtype', type(state).__name__)})")
    if state.dim() != 3 or not all(1 <= int(n) <= MAX_CELLS for n in state.shape):
        raise ValueError(f"{what}: state must be [n0,n1,n2] with every size in [1, {MAX_CELLS}] "
                         f"(got {list(state.shape)}); a 2-D map [n_u,n_v] is the lattice [1,n_u,n_v]")
    dims = tuple(int(n) for n in state.shape)
    if isinstance(origins, torch.Tensor):
        if origins.dtype != torch.int32 or origins.dim() != 2 or origins.shape[1] != 3:
            raise ValueError(f"{what}: origins must be int32 [V,3] (got {origins.dtype} {list(origins.shape)})")
    else:
        o = np.asarray(origins)
        if o.size == 0:
            o = np.zeros((0, 3), dtype=np.int32)
        if o.ndim != 2 or o.shape[1] != 3 or not (np.issubdtype(o.dtype, np.integer) and o.dtype != np.bool_):
            raise ValueError(f"{what}: origins must be integers [V,3] (got {o.dtype} {list(o.shape)})")
        if (np.abs(o.astype(np.int64)) > 0x7fffffff).any():
            raise ValueError(f"{what}: an origin does not fit 32 bits")
        origins = np.ascontiguousarray(o, dtype=np.int32)
    dirs = _dirs(dirs, what)
    r = _int(range_cells, 1, MAX_RANGE, "range_cells", what)
    max_unknown = _int(max_unknown, 0, 0x7fffffff, "max_unknown", what)
    return dims, origins, dirs, r, max_unknown, box_arguments(dirs, r, box, what)


def box_arguments(dirs, r, box, what):
    """`box` as six ints within the cap, None being `view_box(dirs, r)`, or ValueError; the message for a `view_box` over
    the cap names the largest range that fits."""
    if box is None:
        box = view_box(dirs, r)
        if _box_cells(box) > MAX_BOX_CELLS:
            fits, over = 0, r                               # view_box grows with the range: bisect
            while over - fits > 1:
                mid = (fits + over) // 2
                fits, over = (mid, over) if _box_cells(view_box(dirs, mid)) <= MAX_BOX_CELLS else (fits, mid)
            raise ValueError(f"{what}: at range_cells {r} these rays' box {box} holds {_box_cells(box)} cells, over the "
                             f"{MAX_BOX_CELLS} whose visited bits fit in LDS; the largest range that fits is {fits} cells")
    else:
        try:
            box = tuple(int(v) for v in box)
        except (TypeError, ValueError):
            box = ()
        if len(box) != 6 or not all(-0x7fffffff <= box[a] <= 0 <= box[3 + a] <= 0x7fffffff for a in range(3)):
            raise ValueError(f"{what}: box must be (lo0, lo1, lo2, hi0, hi1, hi2) with lo <= 0 <= hi (got {box!r})")
        if _box_cells(box) > MAX_BOX_CELLS:
            raise ValueError(f"{what}: box {box} holds {_box_cells(box)} cells, at most {MAX_BOX_CELLS} fit in LDS")
    return box


@torch.no_grad()
def view_gain(state, origins, dirs, range_cells, max_unknown=0, box=None):
    """int64 [V,4] on the device: per view the distinct unknown, free and solid cells, and their sum, that the rays `dirs`
    (integers [R,3] on the host, where their components are checked; the same for every view) visit from `origins` (int32
    [V,3] cells, host or device) in `state` (uint8 [n0,n1,n2]; on the GPU, or moved there) within `range_cells` (range2 =
    range_cells^2), each ray ending after a solid cell or its `max_unknown`-th unknown one (0: no limit) -- gs_view_gain,
    one launch.  `box` None is `view_box(dirs, range_cells)`, which clips nothing.  Enqueues on the current stream and
    reads nothing back.  ValueError for bad shapes, dtypes, components or a box over the cap, before the device is
    touched."""
    dims, origins, dirs, r, max_unknown, box = gain_arguments(state, origins, dirs, range_cells, max_unknown, box)
    L = _lib.lib()
    dev = state.device if state.is_cuda else torch.device("cuda", torch.cuda.current_device())
    state = state.to(dev).contiguous()
    origins = (origins if isinstance(origins, torch.Tensor) else torch.from_numpy(origins)).to(dev).contiguous()
    dirs_d = torch.from_numpy(dirs).to(dev)
    V = int(origins.shape[0])
    gain = torch.empty((V, 4), dtype=torch.int32, device=dev)                # u32, each at most 2^20
    with torch.cuda.device(dev):
        _lib.check(L.gs_view_gain(_lib.ptr(state), *dims, _lib.ptr(origins), V, _lib.ptr(dirs_d), int(dirs.shape[0]), r * r,
                                  max_unknown, (ctypes.c_int * 6)(*box), _lib.ptr(gain), _lib.stream_ptr(dev)), "view_gain")
    return gain.long()


def camera_arguments(camera, what):
    """(hfov_deg, vfov_deg, n_u, n_v, range_m, pitch_deg) of a camera dict, or ValueError."""
    if not isinstance(camera, dict) or any(k not in CAMERA_KEYS for k in camera):
        raise ValueError(f"{what}: camera is a dict of {CAMERA_KEYS} (got {camera!r})")
    try:
        hfov, vfov = float(camera["hfov_deg"]), float(camera.get("vfov_deg", camera["hfov_deg"]))
        range_m, pitch = float(camera["range_m"]), float(camera.get("pitch_deg", 0.0))
        n_u, n_v = camera["n_u"], camera.get("n_v", 1)
    except (KeyError, TypeError, ValueError):
        raise ValueError(f"{what}: camera needs hfov_deg, n_u and range_m as numbers (got {camera!r})") from None
    if not (0 < hfov < 180 and 0 < vfov < 180 and range_m > 0 and math.isfinite(range_m) and math.isfinite(pitch)):
        raise ValueError(f"{what}: camera fields of view in (0, 180), range_m > 0, pitch_deg finite (got {camera!r})")
    n_u, n_v = _int(n_u, 1, MAX_RAYS, "camera n_u", what), _int(n_v, 1, MAX_RAYS, "camera n_v", what)
    if n_u * n_v > MAX_RAYS:
        raise ValueError(f"{what}: camera of {n_u} x {n_v} rays, at most {MAX_RAYS}")
    return hfov, vfov, n_u, n_v, range_m, pitch


def choice_arguments(n_yaw, min_gain_cells, min_solid_cells, lam, what):
    n_yaw = _int(n_yaw, 1, 4096, "n_yaw", what)
    min_gain_cells = _int(min_gain_cells, 0, 0x7fffffff, "min_gain_cells", what)
    min_solid_cells = _int(min_solid_cells, 0, 0x7fffffff, "min_solid_cells", what)
    lam = float(lam)
    if not (lam >= 0 and math.isfinite(lam)):
        raise ValueError(f"{what}: lam must be a finite number >= 0 per metre (got {lam!r})")
    return n_yaw, min_gain_cells, min_solid_cells, lam


def headings(cam, n_yaw, up_axis, voxel, what):
    """(range_cells, [(yaw, dirs, box)] per heading 2 pi j / n_yaw) of a camera on a lattice of `voxel` metres; ValueError
    for a range below one cell or beyond the lattice's largest, or a box over the cap.  Host only."""
    hfov, vfov, n_u, n_v, range_m, pitch = cam
    range_cells = int(math.floor(range_m / voxel))
    if not 1 <= range_cells <= MAX_RANGE:
        raise ValueError(f"{what}: camera range_m {range_m} is {range_m / voxel} cells of {voxel} m, outside "
                         f"[1, {MAX_RANGE}]")
    out = []
    for j in range(n_yaw):
        yaw = 2.0 * math.pi * j / n_yaw
        dirs = ray_directions(hfov, vfov, n_u, n_v, yaw, math.radians(pitch), up_axis)
        out.append((yaw, dirs, box_arguments(dirs, range_cells, None, what)))
    return range_cells, out


def candidates(cost, up_axis, k0, k1, stride, max_candidates):
    """(cells int32 [V,3], cost int32 [V]) on the device: the cells of the field `cost` (int32 [n0,n1,n2]) below INF on the
    layers k0 .. k1 of `up_axis` whose two other coordinates are multiples of `stride`, by ascending (cost, linear index),
    the first `max_candidates` of them.  torch; the number of candidates is the one read."""
    dims = [int(n) for n in cost.shape]
    ok = cost < INF
    for a in range(3):
        i = torch.arange(dims[a], device=cost.device)
        keep = ((i >= k0) & (i <= k1)) if a == up_axis else (i % stride == 0)
        ok = ok & keep.view([-1 if b == a else 1 for b in range(3)])
    flat = cost.reshape(-1)
    lin = torch.nonzero(ok.reshape(-1))[:, 0]
    order = torch.argsort(flat[lin].long() * (1 << 30) + lin)                # both below 2^30: the keys are distinct
    lin = lin[order][:max_candidates]
    cells = torch.stack([lin // (dims[1] * dims[2]), lin // dims[2] % dims[1], lin % dims[2]], dim=1).to(torch.int32)
    return cells.contiguous(), flat[lin].contiguous()


def gain_table(state, cells, heads, range_cells, max_unknown):
    """int64 [V, n_yaw, 4] on the device: one `view_gain` call per heading, each with its own box."""
    return torch.stack([view_gain(state, cells, dirs, range_cells, max_unknown, box) for _, dirs, box in heads], dim=1)


def choose(table, cost, lin, voxel, lam=0.0, min_gain_cells=1, min_solid_cells=0):
    """((view, heading, score) or None, the number of qualified pairs) from the host table [V, n_yaw, 4] of (unknown, free,
    solid, total), the views' costs in milli-voxels and their linear indices.  A pair qualifies with unknown >=
    min_gain_cells and solid >= min_solid_cells; the largest unknown * voxel^3 * exp(-lam * cost_m) in float64 wins, cost_m
    = cost * voxel / 1000; equal scores go to the lower cost, then the lower linear index, then the lower heading."""
    best, n = None, 0
    for v in range(len(table)):
        cost_m = float(cost[v]) * voxel / 1000.0
        decay = math.exp(-lam * cost_m) if lam else 1.0
        for j in range(len(table[v])):
            unknown, solid = int(table[v][j][0]), int(table[v][j][2])
            if unknown < min_gain_cells or solid < min_solid_cells:
                continue
            n += 1
            key = (-(unknown * voxel ** 3 * decay), int(cost[v]), int(lin[v]), j)
            if best is None or key < best[0]:
                best = (key, v, j)
    return (None if best is None else (best[1], best[2], -best[0][0])), n


def _nothing(n_candidates, gains):
    return {"view_cell": None, "view_point": None, "yaw": None, "yaw_index": None, "gain_cells": 0, "gain_m3": 0.0,
            "free_cells": 0, "solid_cells": 0, "score": 0.0, "n_candidates": int(n_candidates), "n_qualified": 0,
            "gains": gains}


def _pick(state, cells, cost, heads, range_cells, max_unknown, voxel, lam, min_gain_cells, min_solid_cells):
    """The gain table of the candidates, read once with their costs, and the choice on the host: (`_nothing`'s dict filled
    in but for view_point, the chosen cell as a list or None, its cost in milli-voxels)."""
    dims = [int(n) for n in state.shape]
    V, n_yaw = int(cells.shape[0]), len(heads)
    if V == 0:
        return _nothing(0, torch.zeros((0, n_yaw, 4), dtype=torch.int64, device=cells.device)), None, None
    gains = gain_table(state, cells, heads, range_cells, max_unknown)
    c = cells.long()
    lin = (c[:, 0] * dims[1] + c[:, 1]) * dims[2] + c[:, 2]
    host = torch.cat([gains.reshape(V, -1), cost.long()[:, None], lin[:, None]], dim=1).cpu().numpy()        # the one read
    table = host[:, :-2].reshape(V, n_yaw, 4)
    pick, n_qualified = choose(table, host[:, -2], host[:, -1], voxel, lam, min_gain_cells, min_solid_cells)
    out = _nothing(V, gains)
    out["n_qualified"] = n_qualified
    if pick is None:
        return out, None, None
    v, j, score = pick
    out.update(yaw=heads[j][0], yaw_index=j, gain_cells=int(table[v, j, 0]), gain_m3=int(table[v, j, 0]) * voxel ** 3,
               free_cells=int(table[v, j, 1]), solid_cells=int(table[v, j, 2]), score=float(score))
    n1, n2 = dims[1], dims[2]
    cell = int(host[v, -1])
    return out, [cell // (n1 * n2), cell // n2 % n1, cell % n2], int(host[v, -2])


@torch.no_grad()
def esdf_view_candidates(esdf, start, up_axis, height, robot_radius=0.0, stride=4, snap=0.0, max_cost_m=None,
                         max_candidates=4096):
    """`ESDF.view_candidates` (tsdf.py)."""
    what = "ESDF.view_candidates"
    a, k0, k1, _, _ = esdf.slice_arguments(up_axis, height, robot_radius)
    stride = _int(stride, 1, MAX_CELLS, "stride", what)
    max_candidates = _int(max_candidates, 1, 1 << 30, "max_candidates", what)
    (s,), snap_cells, max_cost = esdf.plan_arguments([start], robot_radius, snap, max_cost_m, what)
    passable = esdf.passable(robot_radius)
    s = _plan.snap_cell(passable, s, snap_cells)
    if s is None:
        return (torch.zeros((0, 3), dtype=torch.int32, device=esdf.device),
                torch.zeros(0, dtype=torch.int32, device=esdf.device), None)
    field = _plan.geodesic_field(passable, [s], max_cost)
    field.start_cell = s
    return candidates(field.cost, a, k0, k1, stride, max_candidates) + (field,)


@torch.no_grad()
def esdf_next_view(esdf, start, camera, up_axis, height, n_yaw=8, robot_radius=0.0, stride=4, snap=0.0, max_cost_m=None,
                   max_candidates=4096, max_unknown=0, min_gain_cells=1, min_solid_cells=0, lam=0.0):
    """`ESDF.next_view` (tsdf.py)."""
    what = "ESDF.next_view"
    cam = camera_arguments(camera, what)
    n_yaw, min_gain_cells, min_solid_cells, lam = choice_arguments(n_yaw, min_gain_cells, min_solid_cells, lam, what)
    max_unknown = _int(max_unknown, 0, 0x7fffffff, "max_unknown", what)
    a = _int(up_axis, 0, 2, "up_axis", what)
    range_cells, heads = headings(cam, n_yaw, a, esdf.voxel, what)
    cells, cost, field = esdf_view_candidates(esdf, start, a, height, robot_radius, stride, snap, max_cost_m,
                                              max_candidates)
    found, cell, cell_cost = _pick(esdf.state, cells, cost, heads, range_cells, max_unknown, esdf.voxel, lam,
                                   min_gain_cells, min_solid_cells)
    out = dict(esdf._no_route(None if field is None else field.start_cell, None, 0 if field is None else field.sweeps),
               **found)
    if cell is None:
        return out
    route = torch.flip(field.path(cell), dims=[0]).contiguous()
    points, clearance = esdf._route(route)
    out.update(reachable=True, cells=route, points=points, length_m=cell_cost * esdf.voxel / 1000.0,
               min_clearance_m=float(clearance.item()), goal_cell=cell, view_cell=cell,
               view_point=[float(esdf.lo[i] + cell[i] * esdf.voxel) for i in range(3)])
    return out


@torch.no_grad()
def next_view_on_map(grid, start_xy, camera, n_yaw=8, stride=4, max_candidates=4096, max_unknown=0, min_gain_cells=1,
                     min_solid_cells=0, lam=0.0):
    """`ESDF.next_view` over the 2-D map `grid` (the dict of `ESDF.occupancy_slice` or `load_map`: cells uint8 [n_u,n_v],
    origin, resolution) from the map point `start_xy`: the lattice is [1,n_u,n_v] with up_axis 0, a cell free when it is
    254, unknown when 205, solid otherwise, the candidates the free cells with a route from the start's cell
    floor((xy - origin) / resolution) whose coordinates are multiples of `stride`, and the camera one row of n_u rays over
    hfov_deg (n_v, vfov_deg and pitch_deg are not used: every direction has d_0 = 0).  -> `plan_on_map`'s dict, the route
    start to view, plus the keys of `ESDF.next_view` with `view_cell` (u, v) and `view_point` the cell's centre (x, y);
    when nothing qualifies, its unreachable shape with `view_cell` None.  ValueError before the device is touched."""
    what = "next_view_on_map"
    cells = grid["cells"]
    cells = cells if isinstance(cells, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(cells))
    if cells.dim() != 2 or cells.dtype != torch.uint8:
        raise ValueError(f"{what}: cells must be uint8 [n_u,n_v] (got {cells.dtype} {list(cells.shape)})")
    res = float(grid["resolution"])
    origin = [float(v) for v in grid["origin"]]
    if not res > 0:
        raise ValueError(f"{what}: resolution must be positive (got {res})")
    hfov, _, n_u, _, range_m, _ = camera_arguments(camera, what)
    n_yaw, min_gain_cells, min_solid_cells, lam = choice_arguments(n_yaw, min_gain_cells, min_solid_cells, lam, what)
    max_unknown = _int(max_unknown, 0, 0x7fffffff, "max_unknown", what)
    stride = _int(stride, 1, MAX_CELLS, "stride", what)
    max_candidates = _int(max_candidates, 1, 1 << 30, "max_candidates", what)
    range_cells, heads = headings((hfov, hfov, n_u, 1, range_m, 0.0), n_yaw, 0, res, what)
    start = _plan.map_cell(cells.shape, origin, res, start_xy, "start_xy", what)
    free = cells == _plan.MAP_FREE
    state = torch.where(free, 1, torch.where(cells == _plan.MAP_UNKNOWN, 0, 2)).to(torch.uint8)[None].contiguous()
    field = _plan.geodesic_field(free[None].contiguous(), [[0, start[0], start[1]]])
    cand, cost = candidates(field.cost, 0, 0, 0, stride, max_candidates)
    found, cell, cell_cost = _pick(state.to(field.device), cand, cost, heads, range_cells, max_unknown, res, lam,
                                   min_gain_cells, min_solid_cells)
    out = dict({"reachable": False, "cells": torch.zeros((0, 2), dtype=torch.int32, device=field.device),
                "points": torch.zeros((0, 2), dtype=torch.float64, device=field.device), "length_m": math.inf,
                "start_cell": start, "goal_cell": None, "sweeps": field.sweeps}, **found)
    if cell is None:
        return out
    route = torch.flip(field.path(cell), dims=[0])[:, 1:].contiguous()
    points = torch.tensor(origin, dtype=torch.float64, device=route.device)[None, :] + (route.double() + 0.5) * res
    out.update(reachable=True, cells=route, points=points, length_m=cell_cost * res / 1000.0, goal_cell=tuple(cell[1:]),
               view_cell=tuple(cell[1:]), view_point=[origin[i] + (cell[1 + i] + 0.5) * res for i in range(2)])
    return out


REPORT_ORDER = ("found", "view_cell", "view_point", "yaw", "yaw_index", "gain_cells", "gain_m3", "free_cells",
                "solid_cells", "score", "length_m", "n_candidates", "n_qualified")
_INT_KEYS = ("yaw_index", "gain_cells", "free_cells", "solid_cells", "n_candidates", "n_qualified")
_HEADER = "Next view into the fused TSDF volume"


def next_view_text(result):
    """The text of map/next_view.txt for `ESDF.next_view`'s dict: two header lines, then `name<TAB>value` for the
    REPORT_ORDER keys with repr() numbers (a cell or point: its numbers separated by blanks; None where no view was found):
    reading the file gives back the numbers bit for bit."""
    head = {k: result[k] for k in REPORT_ORDER if k != "found"}
    head["found"] = result["view_cell"] is not None
    lines = [_HEADER + "'s never-observed space: where to stand (view_cell, the lattice cell; view_point [m]) and which way "
             "to look (yaw [rad] about the up axis, heading yaw_index of the headings tried)",
             "(gain_cells: distinct never-observed cells the camera's rays cross from there before a surface stops them; "
             "gain_m3: their volume; free_cells, solid_cells: the known cells in sight; score: gain_m3 * exp(-lam * "
             "length_m); length_m: the route to the view; n_candidates: cells tried; n_qualified: (cell, heading) pairs "
             "over the thresholds)"]
    for k in REPORT_ORDER:
        v = head[k]
        if v is None:
            text = "None"
        elif k == "found":
            text = repr(bool(v))
        elif k == "view_cell":
            text = " ".join(repr(int(x)) for x in v)
        elif k == "view_point":
            text = " ".join(repr(float(x)) for x in v)
        else:
            text = repr(int(v)) if k in _INT_KEYS else repr(float(v))
        lines.append(f"{k}\t{text}")
    return "\n".join(lines) + "\n"


def parse_next_view(text):
    """next_view_text's inverse: the REPORT_ORDER keys (view_cell a list of ints, view_point a list of floats)."""
    lines = text.splitlines()
    if len(lines) != 2 + len(REPORT_ORDER) or not lines[0].startswith(_HEADER):
        raise ValueError("not a map/next_view.txt")
    result = {}
    for key, line in zip(REPORT_ORDER, lines[2:]):
        name, value = line.split("\t")
        if name != key:
            raise ValueError(f"next_view.txt: expected {key}, found {name}")
        if value == "None":
            result[key] = None
        elif key == "found":
            if value not in ("True", "False"):
                raise ValueError(f"next_view.txt: found is {value!r}")
            result[key] = value == "True"
        elif key == "view_cell":
            result[key] = [int(x) for x in value.split(" ")]
        elif key == "view_point":
            result[key] = [float(x) for x in value.split(" ")]
        else:
            result[key] = int(value) if key in _INT_KEYS else float(value)
    return result
