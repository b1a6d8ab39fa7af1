"""Restatement of csrc/tsdf_objects.hip (include/goslam_hip.h: gs_tsdf_object_mark, gs_tsdf_object_table,
gs_tsdf_object_extents, and gs_frontier_relax's fixed point on their labels) in NumPy.  The mark rule runs over
tests/tsdf_planes_restatement.py's samples with one rounding per operation (np.float32 arrays); the labels come from a
serial flood fill from every unvisited object cell in ascending order (so the cell a fill starts from is its cluster's
smallest index); the table is NumPy int64 over the labelled cells; the extents are the minima and maxima of the encoded
floats.  It knows nothing of bricks, sweeps, waves or atomics.

The kernels are restated here; what lies between them is go_slam_amd/tsdf_objects.py already, and `Field` hands the
restated kernels to that same code (`find_objects_in`), so `find_objects` below is the package's pipeline over restated
kernels.  A volume is tsdf_merge_restatement's dict {"tsdf", "weight", "lo", "voxel", "trunc"}."""
import numpy as np

import tsdf_planes_restatement as PR

F = np.float32
NEIGHBOURS = [(d0, d1, d2) for d0 in (-1, 0, 1) for d1 in (-1, 0, 1) for d2 in (-1, 0, 1) if (d0, d1, d2) != (0, 0, 0)]


def cell_dims(vol):
    return tuple(int(n) - 1 for n in np.shape(vol["tsdf"]))


def mark(vol, planes, cos2, band, min_weight=1.0, s=None):
    """gs_tsdf_object_mark: {"kind": uint8 [cx,cy,cz], "label": int32 [cx,cy,cz] (own index on an object cell, else -1),
    "counts": uint32 [4] (samples, object cells, structure cells, crease cells)}."""
    s = PR.samples(vol, min_weight) if s is None else s
    planes = np.asarray(planes, np.float64).reshape(-1, 4).astype(F)
    N = len(s["is"])
    on = np.full(N, -1, np.int64)
    near = np.full(N, -1, np.int64)
    n_near = np.zeros(N, np.int64)
    for j, pl in enumerate(planes):
        with np.errstate(all="ignore"):
            r = PR.along(s, pl[:3]) - pl[3]
            assert r.dtype == F
            near_j = s["is"] & (np.abs(r) <= F(band))               # a NaN is not near
        on_j = near_j & PR.agrees(s, pl[:3], cos2)
        n_near += near_j
        near[near_j & (near < 0)] = j
        on[on_j & (on < 0)] = j
    structure = (on >= 0) | (n_near >= 2)
    obj = s["is"] & ~structure
    kind = np.zeros(N, np.uint8)
    kind[obj] = 1
    kind[structure] = (2 + np.where(on >= 0, on, near))[structure]
    label = np.where(obj, np.arange(N), -1).astype(np.int32)
    counts = np.array([s["is"].sum(), obj.sum(), structure.sum(), (structure & (on < 0)).sum()], np.uint32)
    dims = cell_dims(vol)
    return {"kind": kind.reshape(dims), "label": label.reshape(dims), "counts": counts}


def labels(label):
    """The fixed point of the labels: int32, -1 off the object cells, else the smallest linear index of the cell's
    26-connected cluster."""
    shape = label.shape
    member = label.reshape(-1) >= 0
    out = np.full(member.shape, -1, np.int32)
    for root in np.flatnonzero(member):                         # ascending
        if out[root] >= 0:
            continue
        out[root] = root
        stack = [np.unravel_index(root, shape)]
        while stack:
            a = stack.pop()
            for d in NEIGHBOURS:
                p = (a[0] + d[0], a[1] + d[1], a[2] + d[2])
                if all(0 <= p[i] < shape[i] for i in range(3)):
                    at = (p[0] * shape[1] + p[1]) * shape[2] + p[2]
                    if member[at] and out[at] < 0:
                        out[at] = root
                        stack.append(p)
    return out.reshape(shape)


def table(kind, label, rows=None):
    """gs_tsdf_object_table: {"root", "size" int32 [K], "sum" int64 [K,3], "sum2" int64 [K,6], "bbox" int32 [K,6], "touch"
    uint32 [K]}, rows by ascending root (the first `rows` of them when given)."""
    shape = label.shape
    cells = np.argwhere(label >= 0).astype(np.int64)            # in ascending linear order
    of = label[label >= 0].astype(np.int64)
    roots = np.unique(of)
    if rows is not None:
        roots = roots[:rows]
        keep = np.isin(of, roots)
        cells, of = cells[keep], of[keep]
    K = len(roots)
    row = np.searchsorted(roots, of)
    size = np.zeros(K, np.int64)
    total, total2 = np.zeros((K, 3), np.int64), np.zeros((K, 6), np.int64)
    bbox = np.concatenate([np.full((K, 3), 1 << 20, np.int64), np.full((K, 3), -1, np.int64)], 1)
    touch = np.zeros(K, np.int64)
    np.add.at(size, row, 1)
    np.add.at(total, row, cells)
    pairs = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
    np.add.at(total2, row, np.stack([cells[:, i] * cells[:, j] for i, j in pairs], 1) if len(cells) else np.zeros((0, 6), np.int64))
    np.minimum.at(bbox[:, :3], row, cells)
    np.maximum.at(bbox[:, 3:], row, cells)
    pad = np.zeros(tuple(n + 2 for n in shape), np.int64)
    pad[1:-1, 1:-1, 1:-1] = kind
    for d in NEIGHBOURS:
        k = pad[cells[:, 0] + 1 + d[0], cells[:, 1] + 1 + d[1], cells[:, 2] + 1 + d[2]]
        np.bitwise_or.at(touch, row, np.where(k >= 2, 1 << np.maximum(k - 2, 0), 0))
    return {"root": roots.astype(np.int32), "size": size.astype(np.int32), "sum": total, "sum2": total2,
            "bbox": bbox.astype(np.int32), "touch": touch.astype(np.uint32)}


def encode(x):
    """e(x): uint32 in the order of the float32 values x."""
    b = np.ascontiguousarray(x, F).view(np.uint32)
    return np.where(b >> 31, b ^ np.uint32(0xffffffff), b ^ np.uint32(0x80000000)).astype(np.uint32)


def extents(vol, label, roots, axes, min_weight=1.0, s=None):
    """gs_tsdf_object_extents: uint32 [rows,3,2]."""
    s = PR.samples(vol, min_weight) if s is None else s
    roots = np.asarray(roots, np.int64)
    K = len(roots)
    axes = np.asarray(axes, np.float64).reshape(K, 3, 3).astype(F)
    of = label.reshape(-1).astype(np.int64)
    row = np.searchsorted(roots, of)
    row[row >= K] = 0
    use = (of >= 0) & s["is"] & (K > 0)
    if K:
        use &= roots[row] == of
    ext = np.empty((K, 3, 2), np.uint32)
    ext[:, :, 0], ext[:, :, 1] = 0xff800000, 0x007fffff
    p = s["p"][use]
    a = axes[row[use]]
    for m in range(3):
        with np.errstate(all="ignore"):
            t = (a[:, m, 0] * p[:, 0] + a[:, m, 1] * p[:, 1]) + a[:, m, 2] * p[:, 2]
        assert t.dtype == F
        e = encode(t)
        np.minimum.at(ext[:, m, 0], row[use], e)
        np.maximum.at(ext[:, m, 1], row[use], e)
    return ext


class Field:
    """go_slam_amd.tsdf_objects' `field` over a restated volume: the kernels as restated above."""

    def __init__(self, vol):
        self.vol = vol
        self.dims, self.lo, self.voxel = np.shape(vol["tsdf"]), np.asarray(vol["lo"], np.float64), vol["voxel"]
        self._samples = {}

    def samples(self, min_weight):
        if min_weight not in self._samples:
            self._samples[min_weight] = PR.samples(self.vol, min_weight)
        return self._samples[min_weight]

    def mark(self, planes, cos2, band, min_weight, max_sweeps):
        m = mark(self.vol, planes, cos2, band, s=self.samples(min_weight))
        return {"kind": m["kind"], "label": labels(m["label"]), "counts": m["counts"].astype(np.int64), "sweeps": 0}

    def table(self, marked):
        t = table(marked["kind"], marked["label"])
        return t, t

    def extents(self, marked, columns, axes, min_weight):
        return extents(self.vol, marked["label"], columns["root"], axes, s=self.samples(min_weight))


def find_objects(vol, planes, **kw):
    """TSDFVolume.find_objects over the restated kernels."""
    from go_slam_amd import tsdf_objects as TO
    return TO.find_objects_in(Field(vol), TO.find_arguments("restatement", vol["voxel"], planes, **kw))
