"""Restatement of csrc/tsdf_planes.hip (include/goslam_hip.h: gs_tsdf_plane_votes, gs_tsdf_plane_offsets,
gs_tsdf_plane_moments) in NumPy, with one rounding per operation: np.float32 arrays for the per-cell arithmetic, np.float64
for the sums, whose order is written out literally (a thread's cells t, t + 256, ... of a chunk, the wave's butterfly, the
four waves as ((w0 + w1) + w2) + w3, the chunks in increasing order).  `chunk` is an argument (tests read
gs_tsdf_align_chunk).

The kernels are restated here; what lies between them is fp64 NumPy in go_slam_amd/tsdf_planes.py already, and `Field`
hands the restated kernels to that same code (`find_planes_in`), so `find_planes` and `upright` below are the package's
pipeline over restated kernels and tests/tsdf_merge_restatement.py's merge.

A volume is tsdf_merge_restatement's dict {"tsdf", "weight", "lo", "voxel", "trunc"}."""
import numpy as np

import tsdf_merge_restatement as MR

F = np.float32
THREADS, WAVE = 256, 64
ROW = 16                                    # sum q 0..2, sum q q^T 3..8, sq 9, inliers 10, agreeing 11, 0 x 4
lerp = MR.lerp


def samples(vol, min_weight=1.0):
    """The surface sample of every cell, in cell order s = (a (ny - 1) + b) (nz - 1) + c: {"is": bool [N], "g", "p":
    float32 [N,3], "gg", "f": float32 [N], "idx": int64 [N,3]}.  Rows that are no sample hold whatever the arithmetic gave."""
    t, w = np.ascontiguousarray(vol["tsdf"], F), np.ascontiguousarray(vol["weight"], F)
    nx, ny, nz = t.shape
    mw, h = F(min_weight), F(0.5)

    def corner(x, i, j, k):
        return x[i:nx - 1 + i, j:ny - 1 + j, k:nz - 1 + k].reshape(-1)

    order = [(i, j, k) for i in (0, 1) for j in (0, 1) for k in (0, 1)]          # v000 v001 v010 .. v111
    with np.errstate(all="ignore"):
        wc = [corner(w, *o) for o in order]
        v = [corner(t, *o) for o in order]
        ok = np.ones(wc[0].shape, bool)
        neg, pos = np.zeros(ok.shape, bool), np.zeros(ok.shape, bool)
        for c in wc:
            ok &= c >= mw
        for c in v:
            ok &= np.abs(c) < F(1)
            neg |= c < F(0)
            pos |= c >= F(0)
        ok &= neg & pos
        v000, v001, v010, v011, v100, v101, v110, v111 = v
        z00, z01, z10, z11 = lerp(v000, v001, h), lerp(v010, v011, h), lerp(v100, v101, h), lerp(v110, v111, h)
        y00, y01, y10, y11 = lerp(v000, v010, h), lerp(v001, v011, h), lerp(v100, v110, h), lerp(v101, v111, h)
        x0, x1 = lerp(z00, z01, h), lerp(z10, z11, h)
        f = lerp(x0, x1, h)
        g = [x1 - x0, lerp(z01, z11, h) - lerp(z00, z10, h), lerp(y01, y11, h) - lerp(y00, y10, h)]
        gg = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]
        ok &= (gg > F(0)) & (f * f <= gg)
        step = f / gg
        idx = np.stack([x.reshape(-1) for x in np.meshgrid(np.arange(nx - 1), np.arange(ny - 1), np.arange(nz - 1),
                                                           indexing="ij")], 1)
        p = [F(vol["lo"][r]) + ((idx[:, r].astype(F) + h) - step * g[r]) * F(vol["voxel"]) for r in range(3)]
    for x in g + p + [gg, f]:
        assert x.dtype == F
    return {"is": ok, "g": np.stack(g, 1), "p": np.stack(p, 1), "gg": gg, "f": f, "idx": idx}


def vote_bins(g, bins):
    """(face, bin of u, bin of v) int64 of normal directions g float32 [N,3] (rows with a zero or NaN g give nonsense)."""
    a = np.abs(g)
    m = np.argmax(a, axis=1)                                   # the first of equal maxima: the lowest axis
    rows = np.arange(len(g))
    with np.errstate(all="ignore"):
        gm = g[rows, m]
        b = np.where(m == 0, 1, 0)
        c = np.where(m == 2, 1, 2)
        am = np.abs(gm)
        u, v = g[rows, b] / am, g[rows, c] / am
        half = F(bins // 2)
        iu = np.minimum(bins - 1, np.floor((u + F(1)) * half).astype(np.int64))
        iv = np.minimum(bins - 1, np.floor((v + F(1)) * half).astype(np.int64))
    return 2 * m + (gm < F(0)), iu, iv


def votes(vol, bins, min_weight=1.0, s=None):
    """gs_tsdf_plane_votes: uint32 [6,bins,bins]."""
    s = samples(vol, min_weight) if s is None else s
    g = s["g"][s["is"]]
    face, iu, iv = vote_bins(g, bins)
    out = np.zeros(6 * bins * bins, np.int64)
    np.add.at(out, (face * bins + iu) * bins + iv, 1)
    return out.reshape(6, bins, bins).astype(np.uint32)


def agrees(s, n, cos2):
    """bool [N]: the samples whose normal direction lies in the cone about n (float32 [3])."""
    g = s["g"]
    with np.errstate(all="ignore"):
        d = (n[0] * g[:, 0] + n[1] * g[:, 1]) + n[2] * g[:, 2]
        return s["is"] & (d > F(0)) & (d * d >= F(cos2) * s["gg"])


def along(s, n):
    p = s["p"]
    with np.errstate(all="ignore"):
        return (n[0] * p[:, 0] + n[1] * p[:, 1]) + n[2] * p[:, 2]


def offsets(vol, normals, o0, cos2, bin_m, n_bins, min_weight=1.0, s=None):
    """gs_tsdf_plane_offsets: uint32 [P,n_bins]."""
    s = samples(vol, min_weight) if s is None else s
    normals = np.asarray(normals, np.float64).reshape(-1, 3).astype(F)
    o0 = np.asarray(o0, np.float64).reshape(-1).astype(F)
    out = np.zeros((len(normals), n_bins), np.int64)
    for j, n in enumerate(normals):
        with np.errstate(all="ignore"):
            kf = np.floor((along(s, n) - o0[j]) / F(bin_m))
            keep = agrees(s, n, cos2) & (kf >= F(0)) & (kf < F(n_bins))
        np.add.at(out[j], kf[keep].astype(np.int64), 1)
    return out.astype(np.uint32)


def chunked_sum(rows, chunk):
    """The contract's order over rows float64 [N,ROW].  Adding the +0.0 of a cell that adds nothing changes no bit: a
    running sum that starts at +0.0 is never -0.0."""
    N = rows.shape[0]
    n_chunks = -(-N // chunk)
    padded = np.zeros((n_chunks * chunk, ROW), np.float64)
    padded[:N] = rows
    rounds = padded.reshape(n_chunks, chunk // THREADS, THREADS, ROW)
    acc = np.zeros((n_chunks, THREADS, ROW), np.float64)
    for r in range(chunk // THREADS):                      # thread t: cells t, t + 256, ...
        acc = acc + rounds[:, r]
    v = acc.reshape(n_chunks, THREADS // WAVE, WAVE, ROW)
    lanes = np.arange(WAVE)
    for m in (32, 16, 8, 4, 2, 1):
        v = v + v[:, :, lanes ^ m]
    tot = ((v[:, 0, 0] + v[:, 1, 0]) + v[:, 2, 0]) + v[:, 3, 0]
    out = tot[0].copy()
    for c in range(1, n_chunks):
        out = out + tot[c]
    return out


def moment_rows(s, plane, cos2, band, ref):
    """float64 [N,16]: what each cell adds to the row of one plane (n, o) float64 [4]."""
    pl = np.asarray(plane, np.float64).astype(F)
    ref = np.asarray(ref).astype(F)
    agree = agrees(s, pl[:3], cos2)
    rows = np.zeros((len(agree), ROW), np.float64)
    with np.errstate(all="ignore"):
        r = along(s, pl[:3]) - pl[3]
        inlier = agree & (np.abs(r) <= F(band))
        q = [(s["p"][:, k] - ref[k]) for k in range(3)]
        assert r.dtype == F and q[0].dtype == F
        qd = [x.astype(np.float64) for x in q]
        rd = r.astype(np.float64)
        rows[:, 0], rows[:, 1], rows[:, 2] = qd
        rows[:, 3], rows[:, 4], rows[:, 5] = qd[0] * qd[0], qd[0] * qd[1], qd[0] * qd[2]
        rows[:, 6], rows[:, 7], rows[:, 8] = qd[1] * qd[1], qd[1] * qd[2], qd[2] * qd[2]
        rows[:, 9] = rd * rd
        rows[:, 10] = 1.0
    rows[~inlier] = 0.0
    rows[:, 11] = agree
    return rows


def moments(vol, planes, cos2, band, ref, chunk, min_weight=1.0, s=None):
    """gs_tsdf_plane_moments: float64 [P,16]."""
    s = samples(vol, min_weight) if s is None else s
    planes = np.asarray(planes, np.float64).reshape(-1, 4)
    out = np.zeros((len(planes), ROW), np.float64)
    for j, plane in enumerate(planes):
        out[j] = chunked_sum(moment_rows(s, plane, cos2, band, ref), chunk)
    return out


class Field:
    """go_slam_amd.tsdf_planes' `field` over a restated volume: the three kernels as restated above."""

    def __init__(self, vol, chunk):
        self.vol, self.chunk = vol, chunk
        self.dims, self.lo, self.voxel = vol["tsdf"].shape, np.asarray(vol["lo"], np.float64), vol["voxel"]
        self._samples = {}

    def samples(self, min_weight):
        if min_weight not in self._samples:
            self._samples[min_weight] = samples(self.vol, min_weight)
        return self._samples[min_weight]

    def votes(self, bins, min_weight):
        return votes(self.vol, bins, s=self.samples(min_weight))

    def offsets(self, normals, o0, cos2, bin_m, n_bins, min_weight):
        return offsets(self.vol, normals, o0, cos2, bin_m, n_bins, s=self.samples(min_weight))

    def moments(self, planes, cos2, band, ref32, min_weight):
        return moments(self.vol, planes, cos2, band, ref32, self.chunk, s=self.samples(min_weight))


def find_planes(vol, chunk, **kw):
    """TSDFVolume.find_planes over the restated kernels."""
    from go_slam_amd import tsdf_planes as TP
    return TP.find_planes_in(Field(vol, chunk), TP.find_arguments("restatement", vol["voxel"], **kw))


def upright_lattice(vol, T, voxel=None):
    """(dims, lo float64 [3]) of `union_volume([vol], [T])`'s lattice: the box of the moved corners."""
    from go_slam_amd import tsdf_planes as TP
    from go_slam_amd.tsdf import lattice
    T = np.asarray(T, np.float64)
    corners = TP.box_corners(vol["tsdf"].shape, vol["lo"], vol["voxel"]) @ T[:3, :3].T + T[:3, 3]
    _, lo, dims, _ = lattice(np.stack([corners.min(0), corners.max(0)], 1), vol["voxel"] if voxel is None else voxel,
                             vol["trunc"], "upright_lattice")
    return dims, lo


def upright(vol, T, dims=None, lo=None, max_weight=64.0):
    """TSDFVolume.upright's resampling under the world-to-map transform T [4,4]: tsdf_merge_restatement's merge of `vol`
    into the empty lattice (dims, lo) (None: `upright_lattice`)."""
    if dims is None:
        dims, lo = upright_lattice(vol, T)
    src = {k: v for k, v in vol.items() if k != "colors"}
    empty = MR.empty_volume(dims, lo, vol["voxel"], vol["trunc"], colors=False)
    return MR.merge(empty, src, MR.inverse(np.asarray(T, np.float64)[:3]), max_weight=max_weight)
