"""Projective TSDF fusion from its definition, in float64: the referee of tests/test_tsdf_fusion_model_cpu.py and
tests/test_tsdf_fusion_numerics_gpu.py.  It shares no code with tsdf_restatement.py or tsdf_live_restatement.py and is
not written from the operation list of include/goslam_hip.h; it imports nothing but NumPy.

The definition.  A frame has a world-to-camera matrix M (4 x 4, homogeneous, last row 0 0 0 1), pinhole intrinsics
(fx, fy, cx, cy), a depth image (metres along the optical axis, <= 0: no measurement), an optional mask (0: dropped) and
an optional RGB image.  A lattice point P = lo + idx * voxel has camera coordinates (x, y, z, 1) = M (P, 1).  It projects
to (u, v) = (fx x / z + cx, fy y / z + cy); pixel (iu, iv) covers the half-open unit square [iu - 1/2, iu + 1/2) x
[iv - 1/2, iv + 1/2) about its centre.  The frame OBSERVES the point when z > 1e-3, the projection falls in a pixel of
the image, that pixel has d > 0 and is not masked, and sdf = d - z >= -trunc (the point is not hidden further than one
truncation behind the surface).  The observation is s = min(1, sdf / trunc) and, when sdf <= trunc (the point is not
in free space far in front of the surface), the pixel's colour.  Outcomes: 0 not observed, 1 observed, 2 observed with
colour.  Everything is evaluated in float64 from the float32 inputs the kernel receives (the matrices, the depth, the
images, and lo, voxel, trunc and the intrinsics rounded to float32 as the C call rounds them).

The margin and the bound.  u = 2^-24.  A float32 evaluation rounds every operation once: a result r carries u |r| of its
own plus what its operands carried, to first order.  The quantities a decision compares, with the bound of their float32
evaluation in any order of the same operations:

    p_a = lo_a + idx * voxel                     E(p_a) = u (|idx voxel| + |p_a|)                    (product, sum)
    x, y, z = r0 px + r1 py + r2 pz + t          E(row) = 4 u (|r0 px| + |r1 py| + |r2 pz| + |t|) + sum |r_j| E(p_j)
                                                 (a term passes through at most one product and three sums)
    q = x / z                                    E(q) = (E(x) + |q| E(z)) / |z| + u |q|
    u = fx q + cx                                E(u) = fx E(q) + u |fx q| + u |u|
    u + 1/2                                      E = E(u) + u |u + 1/2|          (and the same in v with fy, cy, y)
    sdf = d - z                                  E(sdf) = E(z) + u |sdf|         (d is an input: exact)
    r = sdf / trunc                              E(r) = E(sdf) / trunc + u |r|   (trunc is an input: exact)
    s = min(1, r)                                E(s) = E(r)                     (min does not enlarge an error)

The comparisons of a pair and their distances from the threshold: z against 1e-3 (|z - 1e-3|, bound E(z)); u + 1/2 and
v + 1/2 against the integers on both sides, which are the pixel's four edges and, for the outermost pixels, the image's
borders (the distance to the nearer integer; for a projection outside the image the distance to the image on an axis that
is outside, since one axis outside settles "not observed"); d > 0 and the mask are exact and never undecided; sdf against
-trunc and against +trunc (bound E(sdf)); r against 1 (bound E(r)).  A comparison is only made when the ones before it
let the point through, as in the definition.  The pair's `margin` and `bound` are those of its most critical comparison
(the smallest margin / bound); the pair is DECIDED when margin > bound: no float32 evaluation within its bounds can then
take another branch than this model.  A lattice point is CLEAN when all its pairs are decided.  No constant is chosen.
"""
import numpy as np

U = 2.0 ** -24
Q_S = 16384.0               # gs_tsdf_accumulate's quantum of s
Q_RGB = 255.0               # and of a colour


def f32(x):
    """a python number as the C call's float argument, in float64"""
    return np.float64(np.float32(x))


def homogeneous(w2c):
    """[K,3,4] float32 -> [K,4,4] float64"""
    w2c = np.asarray(w2c, np.float32).astype(np.float64)
    M = np.zeros((len(w2c), 4, 4))
    M[:, :3, :] = w2c
    M[:, 3, 3] = 1.0
    return M


def lattice_points(dims, lo, voxel):
    """(P float64 [N,4] homogeneous, E float64 [N,3]: the float32 bound of each coordinate), x slowest"""
    ax, err = [], []
    for a in range(3):
        step = np.arange(dims[a], dtype=np.float64) * f32(voxel)
        p = f32(lo[a]) + step
        ax.append(p)
        err.append(U * (np.abs(step) + np.abs(p)))
    P = np.stack([g.reshape(-1) for g in np.meshgrid(*ax, indexing="ij")] + [np.ones(int(np.prod(dims)))], 1)
    E = np.stack([g.reshape(-1) for g in np.meshgrid(*err, indexing="ij")], 1)
    return P, E


def observe(depth, w2c, intr, dims, lo, voxel, trunc, images=None, mask=None):
    """Every (frame, lattice point) pair -> dict of [K,N] arrays (N = nx ny nz, x slowest): "outcome" int8 (0, 1, 2),
    "s" and "s_bound" float64 (where outcome > 0), "iu", "iv" int64 (the pixel, where one was chosen), "z" float64,
    "margin", "bound" float64 of the critical comparison, "decided" bool; "rgb" float64 [K,N,3] (where outcome == 2) when
    images are given."""
    depth = np.asarray(depth, np.float32).astype(np.float64)
    K, H, W = depth.shape
    fx, fy, cx, cy = (f32(v) for v in intr)
    tr, near = f32(trunc), f32(1e-3)
    M = homogeneous(w2c)
    P, EP = lattice_points(dims, lo, voxel)
    N = len(P)
    out = {"outcome": np.zeros((K, N), np.int8), "s": np.zeros((K, N)), "s_bound": np.zeros((K, N)),
           "iu": np.zeros((K, N), np.int64), "iv": np.zeros((K, N), np.int64), "z": np.zeros((K, N)),
           "margin": np.full((K, N), np.inf), "bound": np.zeros((K, N)), "decided": np.ones((K, N), bool)}
    if images is not None:
        out["rgb"] = np.zeros((K, N, 3))
    for f in range(K):
        cam = P @ M[f].T                                     # [N,4]: x, y, z, 1
        mag = np.abs(P[:, None, :]) * np.abs(M[f][None, :, :])          # [N,4 rows,4 terms]
        E = 4 * U * mag.sum(2)[:, :3] + EP @ np.abs(M[f][:3, :3]).T     # [N,3]: E(x), E(y), E(z)
        x, y, z = cam[:, 0], cam[:, 1], cam[:, 2]
        margin, bound, crit = np.full(N, np.inf), np.zeros(N), np.full(N, np.inf)

        def consider(who, m, b):
            """a comparison with margins m and bounds b at the points `who`: it becomes the pair's critical one where
            its m / b is the smallest so far"""
            with np.errstate(all="ignore"):
                r = np.where(b > 0, m / b, np.where(m > 0, np.inf, 0.0))
            worse = r < crit[who]
            sel = who[worse]
            crit[sel], margin[sel], bound[sel] = r[worse], m[worse], b[worse]

        alive = np.arange(N)
        consider(alive, np.abs(z - near), E[:, 2])
        alive = alive[z > near]
        with np.errstate(all="ignore"):
            xa, ya, za = x[alive], y[alive], z[alive]
            qx, qy = xa / za, ya / za
            uu, vv = fx * qx + cx, fy * qy + cy
            Eu = fx * ((E[alive, 0] + np.abs(qx) * E[alive, 2]) / za + U * np.abs(qx)) + U * np.abs(fx * qx) + U * np.abs(uu)
            Ev = fy * ((E[alive, 1] + np.abs(qy) * E[alive, 2]) / za + U * np.abs(qy)) + U * np.abs(fy * qy) + U * np.abs(vv)
            uh, vh = uu + 0.5, vv + 0.5
            Eu, Ev = Eu + U * np.abs(uh), Ev + U * np.abs(vh)
        pu, pv = np.floor(uh), np.floor(vh)
        inside = (pu >= 0) & (pu < W) & (pv >= 0) & (pv < H)
        # outside: the distance to the image on the axis that is most safely outside decides
        out_u = np.where(uh < 0, -uh, np.where(uh >= W, uh - W, -np.inf))
        out_v = np.where(vh < 0, -vh, np.where(vh >= H, vh - H, -np.inf))
        with np.errstate(all="ignore"):
            by_u = np.where(np.isfinite(out_u), out_u / Eu, -np.inf) >= np.where(np.isfinite(out_v), out_v / Ev, -np.inf)
        o = ~inside
        consider(alive[o], np.where(by_u, out_u, out_v)[o], np.where(by_u, Eu, Ev)[o])
        # inside: both axes must stay in their pixel
        i = inside
        consider(alive[i], np.minimum(uh - pu, pu + 1 - uh)[i], Eu[i])
        consider(alive[i], np.minimum(vh - pv, pv + 1 - vh)[i], Ev[i])
        alive, iu, iv = alive[i], pu[i].astype(np.int64), pv[i].astype(np.int64)
        out["iu"][f, alive], out["iv"][f, alive] = iu, iv
        ok = depth[f, iv, iu] > 0
        if mask is not None:
            ok &= np.asarray(mask[f], np.float32)[iv, iu] != 0
        alive, iu, iv = alive[ok], iu[ok], iv[ok]
        sdf = depth[f, iv, iu] - z[alive]
        Esdf = E[alive, 2] + U * np.abs(sdf)
        consider(alive, np.abs(sdf + tr), Esdf)
        seen = sdf >= -tr
        alive, iu, iv, sdf, Esdf = alive[seen], iu[seen], iv[seen], sdf[seen], Esdf[seen]
        r = sdf / tr
        Er = Esdf / tr + U * np.abs(r)
        consider(alive, np.abs(sdf - tr), Esdf)
        consider(alive, np.abs(r - 1.0), Er)
        out["outcome"][f, alive] = np.where(sdf <= tr, 2, 1)
        out["s"][f, alive], out["s_bound"][f, alive] = np.minimum(1.0, r), Er
        if images is not None:
            c = sdf <= tr
            out["rgb"][f, alive[c]] = np.asarray(images[f], np.float32).astype(np.float64)[:, iv[c], iu[c]].T
        out["z"][f], out["margin"][f], out["bound"][f] = z, margin, bound
        out["decided"][f] = margin > bound
    return out


def clean_points(obs):
    """bool [N]: every pair of the point is decided"""
    return obs["decided"].all(axis=0)


def shares(obs):
    """(undecided pairs / observed pairs, points that are not clean / points, observed points / points)"""
    observed = obs["outcome"] > 0
    return (float((~obs["decided"]).sum()) / max(1, int(observed.sum())), float((~clean_points(obs)).mean()),
            float(observed.any(axis=0).mean()))


def running_mean(obs, max_weight, color=True, frames=None):
    """gs_tsdf_integrate's recursion over the frames in order (or over `frames`), in float64, from a fresh volume (tsdf 1,
    weight 0, colour 0).  An observation does  w1 = w + 1 ; tsdf = (tsdf w + s) / w1 ; colour = (colour w + rgb) / w1
    when it carries colour ; w = min(w1, max_weight): with the cap a recursion, not a mean.
    -> {"tsdf", "weight" [N], "colors" [3,N], "tsdf_bound" [N], "colors_bound" [3,N]}.

    The bound of the float32 recursion, carried along: if the stored value carries e and the observation e_s, the new
    value (t w + s) / w1 carries (w e + e_s) / w1 from them (w, w1 are small integers, exact) plus u |t w| for the product,
    u |t w + s| for the sum, both divided by w1, plus u |new| for the quotient.  e_s = E(s) for the distance and 0 for a
    colour (an input)."""
    K, N = obs["outcome"].shape
    mw = f32(max_weight)
    t, w, et = np.ones(N), np.zeros(N), np.zeros(N)
    c, ec = np.zeros((3, N)), np.zeros((3, N))
    color = color and "rgb" in obs
    for f in (range(K) if frames is None else frames):
        hit = obs["outcome"][f] > 0
        w0, w1 = w[hit], w[hit] + 1.0
        s = obs["s"][f, hit]
        new = (t[hit] * w0 + s) / w1
        et[hit] = (w0 * et[hit] + obs["s_bound"][f, hit] + U * np.abs(t[hit] * w0) + U * np.abs(t[hit] * w0 + s)) / w1 \
            + U * np.abs(new)
        t[hit] = new
        if color:
            g = obs["outcome"][f] == 2
            g0, g1 = w[g], w[g] + 1.0
            rgb = obs["rgb"][f, g].T
            newc = (c[:, g] * g0 + rgb) / g1
            ec[:, g] = (g0 * ec[:, g] + U * np.abs(c[:, g] * g0) + U * np.abs(c[:, g] * g0 + rgb)) / g1 + U * np.abs(newc)
            c[:, g] = newc
        w[hit] = np.minimum(w1, mw)
    return {"tsdf": t, "weight": w, "colors": c, "tsdf_bound": et, "colors_bound": ec}


def integer_sums(obs, alive=None, color=True):
    """gs_tsdf_accumulate + gs_tsdf_resolve for the frames `alive` (bool [K]: added and not taken out again; default all).
    An observation adds rint(16384 s) to sum_s and 1 to count and, with colour, rint(255 clamp(rgb, 0, 1)) to sum_rgb and
    1 to count_rgb; taking a frame out subtracts the same integers, so the state is the sum over the frames alive.
    -> {"count", "count_rgb" int64 [N]: exact on clean points; "tsdf" [N]: the float64 mean of s (1 where count = 0),
    "tsdf_bound"; "colors" [3,N]: the mean of the clamped colours (0 where count_rgb = 0), "colors_bound"}.

    The bounds.  16384 s is exact in float32 (a power of two), so an observation's integer over 16384 is within half a
    quantum, 0.5 / 16384, of the float32 s, which is within E(s) of s; the mean of n such numbers is within
    0.5 / 16384 + mean E(s) of the mean of s; resolve's division is in double and its one rounding to float32 adds
    u |tsdf|.  255 c is rounded once before rint: (0.5 + 255 u) / 255 per observation, plus u |colour| for resolve."""
    K, N = obs["outcome"].shape
    alive = np.ones(K, bool) if alive is None else np.asarray(alive, bool)
    hit = (obs["outcome"] > 0) & alive[:, None]
    count = hit.sum(0)
    n = np.maximum(count, 1)
    tsdf = np.where(count > 0, (obs["s"] * hit).sum(0) / n, 1.0)
    bound = np.where(count > 0, 0.5 / Q_S + (obs["s_bound"] * hit).sum(0) / n + U * np.abs(tsdf), 0.0)
    res = {"count": count, "tsdf": tsdf, "tsdf_bound": bound, "count_rgb": np.zeros(N, np.int64),
           "colors": np.zeros((3, N)), "colors_bound": np.zeros((3, N))}
    if color and "rgb" in obs:
        g = (obs["outcome"] == 2) & alive[:, None]
        cn = g.sum(0)
        m = np.maximum(cn, 1)
        clamped = np.clip(obs["rgb"], 0.0, 1.0) * g[:, :, None]
        res["count_rgb"] = cn
        res["colors"] = np.where(cn > 0, clamped.sum(0).T / m, 0.0)
        res["colors_bound"] = np.where(cn > 0, (0.5 + Q_RGB * U) / Q_RGB + U * np.abs(res["colors"]), 0.0)
    return res
