"""What stands in the room: the surface samples of a `TSDFVolume` that lie on none of its structure planes, grouped into
objects, each with its place, its size, how it is turned and what it touches.

`tsdf_planes.find_planes` answers "what is level"; every surface sample that is not floor, wall or ceiling belongs to a
thing.  csrc/tsdf_objects.hip has the kernels: gs_tsdf_object_mark decides per cell of the lattice "object or structure"
(on a structure plane, or in the crease where two of them meet), gs_frontier_relax / gs_frontier_roots label the
26-connected clusters of the object cells, gs_tsdf_object_table folds every cluster into one row of integers (size, first
and second moments of the cell coordinates, box, the planes it touches) and gs_tsdf_object_extents measures every cluster's
sample points along three given axes.  Arithmetic contract: include/goslam_hip.h (gs_tsdf_object_*);
tests/tsdf_objects_restatement.py restates it.

Everything between the kernels is fp64 NumPy (and Python integers) on the host and takes the kernels through a `field`: an
object with `dims`, `lo`, `voxel` and the methods `mark`, `table` and `extents`.  `DeviceField` is the one over a volume on
the GPU; the restatement brings its own, so `find_objects_in` is one code for both.

`structure_planes` states which of `find_planes`' planes are structure, `find_objects` (TSDFVolume.find_objects) returns the
`Objects`, `moved_objects` takes their boxes into another frame and `objects_text` / `parse_objects` write and read
map/objects.txt (tsdf.fuse_from_config, cfg["tsdf"]["objects"]).
"""
import math

import numpy as np

from . import _lib
from . import tsdf_merge as _merge
from . import tsdf_planes as _planes

MAX_PLANES = _planes.MAX_PLANES                  # structure planes of one call
EXT_EMPTY = (0xff800000, 0x007fffff)             # e(+inf), e(-inf): a row no cell entered


# ---- arguments ----------------------------------------------------------------------------------------------------------
def structure_planes(planes, floor=None, min_area_m2=2.0):
    """Which of `find_planes`' planes are structure, by a stated policy: the floor first if one is given (one of `planes`),
    then every other plane with area_m2 >= min_area_m2, in `planes`' order; at most 16.  (`find_planes` also returns the
    large faces of a big box: a plane is structure by its area, not by being a plane.)  -> (the chosen planes, their
    indices into `planes`).  ValueError for bad arguments."""
    what = "structure_planes"
    min_area_m2 = float(min_area_m2)
    if not min_area_m2 >= 0:
        raise ValueError(f"{what}: min_area_m2 must be at least 0 (got {min_area_m2})")
    index = []
    if floor is not None:
        at = [i for i, p in enumerate(planes) if p is floor]
        if not at:
            raise ValueError(f"{what}: floor must be one of planes")
        index.append(at[0])
    for i, p in enumerate(planes):
        _planes._plane(p, what, f"plane {i}")
        if i not in index and float(p.get("area_m2", 0.0)) >= min_area_m2:
            index.append(i)
    index = index[:MAX_PLANES]
    return [planes[i] for i in index], index


def find_arguments(what, voxel, planes, up=None, cone_deg=10.0, band=None, min_cells=16, min_weight=1.0, max_sweeps=65536):
    """The checked arguments of `find_objects`: a dict; cos2, band and min_weight are rounded to fp32 here, as the kernels
    take them; "planes" float64 [P,4] = (n, o); "up" float64 [3] and "up_offset" (None when up is a bare vector).
    ValueError otherwise."""
    try:
        planes = list(planes)
    except TypeError:
        raise ValueError(f"{what}: planes must be a list of planes") from None
    if len(planes) > MAX_PLANES:
        raise ValueError(f"{what}: at most {MAX_PLANES} structure planes (got {len(planes)})")
    rows = [_planes._plane(p, what, f"plane {i}") for i, p in enumerate(planes)]
    if up is None:
        if not rows:
            raise ValueError(f"{what}: without structure planes, up must say where up is")
        up, up_offset = rows[0]
    elif isinstance(up, dict):
        up, up_offset = _planes._plane(up, what, "up")
    else:
        up, up_offset = _planes._vector3(up, what, "up"), None
    cone_deg = float(cone_deg)
    if not 0 < cone_deg < 90:
        raise ValueError(f"{what}: cone_deg must lie in (0, 90) (got {cone_deg})")
    band = float(voxel) if band is None else float(band)
    if not (band > 0 and math.isfinite(band)):
        raise ValueError(f"{what}: band must be positive and finite, in metres (got {band})")
    if isinstance(min_cells, bool) or int(min_cells) != min_cells or int(min_cells) < 1:
        raise ValueError(f"{what}: min_cells must be at least 1 (got {min_cells})")
    min_weight = float(min_weight)
    if not math.isfinite(min_weight):
        raise ValueError(f"{what}: min_weight must be finite (got {min_weight})")
    if isinstance(max_sweeps, bool) or not isinstance(max_sweeps, (int, np.integer)) or int(max_sweeps) < 1:
        raise ValueError(f"{what}: max_sweeps must be a positive integer (got {max_sweeps!r})")
    return {"planes": np.array([[*n, o] for n, o in rows], np.float64).reshape(-1, 4), "up": up, "up_offset": up_offset,
            "cone_deg": cone_deg, "cos2": float(np.float32(math.cos(math.radians(cone_deg)) ** 2)),
            "band": float(np.float32(band)), "min_cells": int(min_cells), "min_weight": float(np.float32(min_weight)),
            "max_sweeps": int(max_sweeps)}


# ---- the host steps between the kernels -------------------------------------------------------------------------------------
def level_basis(up):
    """float64 [2,3]: two unit vectors that span the plane perpendicular to the unit vector up: the coordinate axis up has
    least of (the lowest on a tie), made perpendicular to up, and up x that."""
    e = np.zeros(3)
    e[int(np.argmin(np.abs(up)))] = 1.0
    e1 = e - float(e @ up) * up
    e1 = e1 / np.linalg.norm(e1)
    return np.stack([e1, np.cross(up, e1)])


def covariance_integers(size, total, total2):
    """size * sum2 - sum (x) sum as a 3 x 3 list of Python integers: size^2 times the covariance of the cell coordinates,
    exact.  total: three integers, total2: the six sums of products 00 01 02 11 12 22."""
    n, s = int(size), [int(v) for v in total]
    q = [int(v) for v in total2]
    full = [[q[0], q[1], q[2]], [q[1], q[3], q[4]], [q[2], q[4], q[5]]]
    return [[n * full[i][j] - s[i] * s[j] for j in range(3)] for i in range(3)]


def object_axes(size, total, total2, up):
    """(axes float64 [3,3] with rows up, long, short; elongation) of one cluster from its exact moments: the covariance
    `covariance_integers`, turned to floats once, is projected onto the plane perpendicular to up (`level_basis`); long is
    the eigenvector of the larger eigenvalue there, its sign such that its largest-magnitude component (the lowest axis on
    a tie) is positive; short = up x long; elongation the ratio of the larger to the smaller eigenvalue, inf when the
    smaller is not positive."""
    C = np.array([[float(v) for v in row] for row in covariance_integers(size, total, total2)], np.float64)
    E = level_basis(up)
    w, V = np.linalg.eigh(E @ C @ E.T)                          # ascending
    long = V[:, 1] @ E
    long = long / np.linalg.norm(long)
    if long[int(np.argmax(np.abs(long)))] < 0:
        long = -long
    elongation = float(w[1] / w[0]) if w[0] > 0 else math.inf
    return np.stack([up, long, np.cross(up, long)]), elongation


def decode_extents(ext):
    """float64 array of the floats that the uint32 array `ext` encodes (gs_tsdf_object_extents' e)."""
    e = np.asarray(ext, np.uint32)
    bits = np.where(e >> 31, e ^ np.uint32(0x80000000), e ^ np.uint32(0xffffffff)).astype(np.uint32)
    return bits.view(np.float32).astype(np.float64)


def touched(mask):
    """The indices of the set bits of a table row's `touch`."""
    return [j for j in range(MAX_PLANES) if int(mask) >> j & 1]


class Objects:
    """`find_objects`' result.  `.kind` uint8 and `.label` int32 over the cell lattice (nx - 1, ny - 1, nz - 1) and `.counts`
    int64 [4] (samples, object cells, structure cells, crease cells), where the field keeps them (`DeviceField`: on the
    device); the table's columns, one row per cluster by ascending root -- `.root`, `.size` int32 [K], `.sum` int64 [K,3],
    `.sum2` int64 [K,6], `.bbox` int32 [K,6] (mins, then maxes), `.touch` int32 [K] (bit j: structure plane j) -- `.ext`
    uint32 [K,3,2] on the host (the extents along `.axes` float64 [K,3,3], encoded; the rows of clusters below min_cells
    are measured along up and `level_basis`), `.n_clusters` = K, `.sweeps`, `.up`, `.up_offset`, `.planes` float64 [P,4]
    and `.boxes`, the clusters of at least min_cells cells by descending size (ties: ascending root), each a dict: root,
    cells, axes float64 [3,3] (rows up, long, short), centre float64 [3], size_m float64 [3] (along up, long, short),
    elongation, touches (indices of the structure planes), bbox_cells (six integers) and above_m (the lowest and highest
    extent along up above the plane `up` came from; None for a bare vector)."""

    def __init__(self, marked, columns, ext, axes, boxes, args):
        self.kind, self.label, self.counts, self.sweeps = marked["kind"], marked["label"], marked["counts"], int(marked["sweeps"])
        for name in ("root", "size", "sum", "sum2", "bbox", "touch"):
            setattr(self, name, columns[name])
        self.ext, self.axes, self.boxes = ext, axes, boxes
        self.n_clusters = int(ext.shape[0])
        self.up, self.up_offset, self.planes = args["up"], args["up_offset"], args["planes"]


def find_objects_in(field, args):
    """`find_objects` over a `field` (see the module's text) with `find_arguments`' dict."""
    marked = field.mark(args["planes"], args["cos2"], args["band"], args["min_weight"], args["max_sweeps"])
    host, columns = field.table(marked)
    K = int(host["root"].shape[0])
    up = args["up"]
    plain = np.stack([up, *level_basis(up)])
    axes, elongation = np.tile(plain, (K, 1, 1)), np.full(K, math.inf)
    kept = [i for i in range(K) if int(host["size"][i]) >= args["min_cells"]]
    for i in kept:
        axes[i], elongation[i] = object_axes(host["size"][i], host["sum"][i], host["sum2"][i], up)
    ext = np.asarray(field.extents(marked, columns, axes, args["min_weight"]), np.uint32).reshape(K, 3, 2)
    span = decode_extents(ext)
    boxes = []
    for i in sorted(kept, key=lambda i: (-int(host["size"][i]), int(host["root"][i]))):
        mid = 0.5 * (span[i, :, 0] + span[i, :, 1])
        box = {"root": int(host["root"][i]), "cells": int(host["size"][i]), "axes": axes[i].copy(), "centre": mid @ axes[i],
               "size_m": span[i, :, 1] - span[i, :, 0], "elongation": float(elongation[i]),
               "touches": touched(host["touch"][i]), "bbox_cells": [int(v) for v in host["bbox"][i]], "above_m": None}
        if args["up_offset"] is not None:
            box["above_m"] = (float(span[i, 0, 0] - args["up_offset"]), float(span[i, 0, 1] - args["up_offset"]))
        boxes.append(box)
    return Objects(marked, columns, ext, axes, boxes, args)


# ---- the kernels over a volume on the GPU -------------------------------------------------------------------------------
TABLE_ROW_BYTES = 8 * 3 + 8 * 6 + 4 + 4 + 4 * 6 + 4          # sum, sum2, root, size, bbox, touch


class DeviceField:
    """gs_tsdf_object_* and gs_frontier_relax / _roots over a TSDFVolume, on the current stream.  Host reads: `mark` one per
    batch of sweeps and the 4-byte root count, `table` one (the columns lie in one buffer), `extents` one."""

    def __init__(self, vol):
        self.vol, self.dims, self.lo, self.voxel = vol, vol.dims, vol.lo, vol.voxel
        self.cells = tuple(int(n) - 1 for n in vol.dims)

    def _lattice(self):
        v = self.vol
        return [_lib.ptr(v.tsdf), _lib.ptr(v.weight), *v.dims, float(v.lo[0]), float(v.lo[1]), float(v.lo[2]), v.voxel]

    def mark(self, planes, cos2, band, min_weight, max_sweeps):
        import torch
        from . import plan as _plan
        what = "TSDFVolume.find_objects"
        dev, L, cells = self.vol.device, _lib.lib(), self.cells
        p_d = torch.as_tensor(np.ascontiguousarray(planes, np.float64)).to(dev)
        kind = torch.empty(cells, dtype=torch.uint8, device=dev)
        label = torch.empty(cells, dtype=torch.int32, device=dev)
        counts = torch.empty(4, dtype=torch.int32, device=dev)                # u32, each below 2^30
        flags = torch.empty(L.gs_frontier_flags_bytes(*cells), dtype=torch.uint8, device=dev)
        changed = torch.empty(_plan.SWEEP_BATCH, dtype=torch.int32, device=dev)
        ws_bytes = L.gs_frontier_workspace_bytes(*cells)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        n_roots = torch.empty(1, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            stream = _lib.stream_ptr(dev)
            _lib.check(L.gs_tsdf_object_mark(*self._lattice(), min_weight, _lib.ptr(p_d), int(p_d.shape[0]), cos2, band,
                                             _lib.ptr(kind), _lib.ptr(label), _lib.ptr(counts), _lib.ptr(flags), stream),
                       f"{what} (mark)")
            sweeps = _plan.sweep_to_fixed_point(
                lambda sweep0, k: _lib.check(L.gs_frontier_relax(*cells, _lib.ptr(label), _lib.ptr(flags), sweep0, k,
                                                                 _lib.ptr(changed), stream), f"{what} (relax)"),
                changed, max_sweeps, what)
            _lib.check(L.gs_frontier_roots(_lib.ptr(label), *cells, _lib.ptr(ws), ws_bytes, _lib.ptr(n_roots), stream),
                       f"{what} (roots)")
            K = int(n_roots.item())                                           # the read that sizes the table
        return {"kind": kind, "label": label, "counts": counts.long(), "sweeps": sweeps, "K": K, "workspace": ws}

    def table(self, marked):
        import torch
        dev, L, K = self.vol.device, _lib.lib(), marked["K"]
        buf = torch.empty(K * TABLE_ROW_BYTES, dtype=torch.uint8, device=dev)

        def columns(b):
            at, out = 0, {}
            for name, dtype, width in (("sum", torch.int64, 3), ("sum2", torch.int64, 6), ("root", torch.int32, 1),
                                       ("size", torch.int32, 1), ("bbox", torch.int32, 6), ("touch", torch.int32, 1)):
                n = K * width * (8 if dtype == torch.int64 else 4)
                col = b[at:at + n].view(dtype)
                out[name] = col.reshape(K, width) if width > 1 else col
                at += n
            return out
        cols = columns(buf)
        if K > 0:
            with torch.cuda.device(dev):
                _lib.check(L.gs_tsdf_object_table(_lib.ptr(marked["kind"]), _lib.ptr(marked["label"]), *self.cells,
                                                  _lib.ptr(marked["workspace"]), marked["workspace"].numel(), K, K,
                                                  _lib.ptr(cols["root"]), _lib.ptr(cols["size"]), _lib.ptr(cols["sum"]),
                                                  _lib.ptr(cols["sum2"]), _lib.ptr(cols["bbox"]), _lib.ptr(cols["touch"]),
                                                  _lib.stream_ptr(dev)), "TSDFVolume.find_objects (table)")
        host = {k: v.numpy() for k, v in columns(buf.cpu()).items()}          # the table's one read
        return host, cols

    def extents(self, marked, columns, axes, min_weight):
        import torch
        dev, L, K = self.vol.device, _lib.lib(), marked["K"]
        a_d = torch.as_tensor(np.ascontiguousarray(axes, np.float64)).to(dev)
        ext = torch.empty((K, 3, 2), dtype=torch.int32, device=dev)           # u32
        if K > 0:
            with torch.cuda.device(dev):
                _lib.check(L.gs_tsdf_object_extents(*self._lattice(), min_weight, _lib.ptr(marked["label"]),
                                                    _lib.ptr(columns["root"]), K, _lib.ptr(a_d), _lib.ptr(ext),
                                                    _lib.stream_ptr(dev)), "TSDFVolume.find_objects (extents)")
        return ext.cpu().numpy().view(np.uint32)


def find_objects(vol, planes, up=None, cone_deg=10.0, band=None, min_cells=16, min_weight=1.0, max_sweeps=65536):
    """The objects of the volume: an `Objects`.  `planes` are the structure planes (`structure_planes` of `find_planes`'
    planes; at most 16).  A surface sample (see `tsdf_planes.find_planes`) is structure when it lies within `band`
    (default: one voxel) of a structure plane and its normal direction within cone_deg of the plane's, or within `band` of
    two structure planes whatever its direction: the crease where floor and wall meet, whose in-between normals agree
    with neither.  Every other sample is an object cell; their 26-connected clusters are labelled by brick sweeps
    (gs_frontier_relax through `plan.sweep_to_fixed_point`; RuntimeError after max_sweeps) and tabulated, and every
    cluster of at least min_cells cells becomes a box: its axes from the exact integer moments of its cells with `up` (a
    unit vector, or a plane whose normal it is; default: the first structure plane) as the first, its extents from its
    samples' points along them.  Without planes every sample is an object cell and the clusters are the surface's
    connected pieces.  ValueError for bad arguments, before the library or the device is reached."""
    what = "TSDFVolume.find_objects"
    _merge._volume(vol, what, "self")
    args = find_arguments(what, vol.voxel, planes, up, cone_deg, band, min_cells, min_weight, max_sweeps)
    return find_objects_in(DeviceField(vol), args)


# ---- another frame, and map/objects.txt -------------------------------------------------------------------------------------
def moved_objects(objects, T):
    """The boxes of `objects` (an `Objects` or a list of boxes) in the frame T [4,4] maps theirs to (a rigid transform, such
    as `tsdf_planes.upright_transform`'s world to map): axes and centre are moved; sizes, elongation, cells, touches,
    above_m and bbox_cells (cells of the lattice the objects were found in) stay.  ValueError for a T that is not rigid."""
    T = np.asarray(T, np.float64)
    _merge.transforms34(T, "moved_objects")
    R, t = T[:3, :3], T[:3, 3]
    out = []
    for b in (objects.boxes if isinstance(objects, Objects) else objects):
        out.append(dict(b, axes=np.asarray(b["axes"], np.float64) @ R.T, centre=R @ np.asarray(b["centre"], np.float64) + t))
    return out


_OBJECTS_HEAD = "Objects of the fused TSDF volume"
_FRAMES = ("world", "map")
_TOKENS = 2 + 6 + 1 + 9 + 3 + 3 + 1 + 2


def _block(frame, boxes):
    lines = [f"frame\t{frame}", f"objects\t{len(boxes)}"]
    for b in boxes:
        ints = [b["root"], b["cells"], *b["bbox_cells"], sum(1 << j for j in b["touches"])]
        above = ["None", "None"] if b["above_m"] is None else [repr(float(v)) for v in b["above_m"]]
        vals = [*np.asarray(b["axes"], np.float64).reshape(-1), *b["centre"], *b["size_m"], b["elongation"]]
        lines.append(" ".join([repr(int(v)) for v in ints] + [repr(float(v)) for v in vals] + above))
    return lines


def objects_text(boxes, moved=None):
    """The text of map/objects.txt: two header lines, then a block in the run's world and, with `moved`, a second one in
    the map frame; a block is its frame, its number of objects and a line per object.  Numbers are written with repr():
    `parse_objects` gives them back bit for bit."""
    lines = [_OBJECTS_HEAD + ": the clusters of surface samples that lie on no structure plane, by descending size, each "
             "with the box of its samples along the axes up, long and short",
             "(per object: root cells, the cell box min0 min1 min2 max0 max1 max2, touch (bit j: structure plane j), the axes "
             "up long short as nine numbers, centre, size_m along the three axes, elongation, above_m lowest highest "
             "(None None without a floor))"]
    lines += _block(_FRAMES[0], boxes)
    if moved is not None:
        lines += _block(_FRAMES[1], moved)
    return "\n".join(lines) + "\n"


def parse_objects(text):
    """objects_text's inverse: (boxes, moved or None)."""
    lines = text.splitlines()
    if len(lines) < 4 or not lines[0].startswith(_OBJECTS_HEAD):
        raise ValueError("not a map/objects.txt")
    blocks, at = [], 2
    while at < len(lines):
        if len(blocks) == 2 or at + 1 >= len(lines) or lines[at] != f"frame\t{_FRAMES[len(blocks)]}" or \
                not lines[at + 1].startswith("objects\t"):
            raise ValueError("map/objects.txt: a block does not begin with its frame and its number of objects")
        n = int(lines[at + 1].split("\t")[1])
        rows = [line.split(" ") for line in lines[at + 2:at + 2 + n]]
        if len(rows) != n or any(len(r) != _TOKENS for r in rows):
            raise ValueError("map/objects.txt: the objects do not match their number")
        boxes = []
        for r in rows:
            i, f = [int(v) for v in r[:9]], [float(v) for v in r[9:25]]
            boxes.append({"root": i[0], "cells": i[1], "axes": np.array(f[:9], np.float64).reshape(3, 3),
                          "centre": np.array(f[9:12], np.float64), "size_m": np.array(f[12:15], np.float64),
                          "elongation": f[15], "touches": touched(i[8]), "bbox_cells": i[2:8],
                          "above_m": None if r[25] == "None" else (float(r[25]), float(r[26]))})
        blocks.append(boxes)
        at += 2 + n
    if not blocks:
        raise ValueError("map/objects.txt: no block")
    return blocks[0], (blocks[1] if len(blocks) == 2 else None)
