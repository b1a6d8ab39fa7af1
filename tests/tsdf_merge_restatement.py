"""Restatement of csrc/tsdf_merge.hip (include/goslam_hip.h: gs_tsdf_register_system, gs_tsdf_merge) in NumPy, with one
rounding per operation: np.float32 arrays for the per-sample arithmetic, np.float64 for the sums.  The summation order
and the step are tests/tsdf_align_restatement.py's (`chunked_sum`, `step`): the contract says they are the same.  It
imports nothing from the package; `chunk` is an argument (tests read gs_tsdf_align_chunk).

A volume is a dict {"tsdf", "weight": float32 [nx,ny,nz], "colors": float32 [3,nx,ny,nz] or absent, "lo": three numbers,
"voxel", "trunc"}."""
import numpy as np

import tsdf_align_restatement as AR

F = np.float32
ROW = AR.ROW
lerp = AR.lerp


def volume(tsdf, weight, lo, voxel, trunc, colors=None):
    v = {"tsdf": np.ascontiguousarray(tsdf, F), "weight": np.ascontiguousarray(weight, F), "lo": tuple(float(x) for x in lo),
         "voxel": float(voxel), "trunc": float(trunc)}
    if colors is not None:
        v["colors"] = np.ascontiguousarray(colors, F)
    return v


def empty_volume(dims, lo, voxel, trunc, colors=True):
    return volume(np.ones(dims, F), np.zeros(dims, F), lo, voxel, trunc, np.zeros((3,) + tuple(dims), F) if colors else None)


def cell(points, vol, F=F):
    """(g, a, inside, at) of float32 (`F`) world points [three arrays] in `vol`: g = (p - lo) / voxel, a = floorf(g), inside = 0
    <= a < float(n - 1) on every axis (a NaN fails), at = the linear index of the cell's first corner (0 where outside)."""
    dims = vol["tsdf"].shape
    lo, voxel = [F(v) for v in vol["lo"]], F(vol["voxel"])
    g = [(points[r] - lo[r]) / voxel for r in range(3)]
    a = [np.floor(x) for x in g]
    inside = np.ones(g[0].shape, bool)
    for x, n in zip(a, dims):
        inside &= (x >= 0) & (x < F(n - 1))
    ai = [np.where(inside, x, F(0)).astype(np.int64) for x in a]
    return g, a, inside, (ai[0] * dims[1] + ai[1]) * dims[2] + ai[2]


def corner_offsets(dims):
    return [(i * dims[1] + j) * dims[2] + k for i in (0, 1) for j in (0, 1) for k in (0, 1)]         # v000 v001 .. v111


def trilinear(c, sx, sy, sz):
    """The value of the corners c = (v000 .. v111) by lerps z, y, x."""
    z00, z01, z10, z11 = lerp(c[0], c[1], sz), lerp(c[2], c[3], sz), lerp(c[4], c[5], sz), lerp(c[6], c[7], sz)
    return lerp(lerp(z00, z01, sy), lerp(z10, z11, sy), sx)


def strided_samples(dims, stride):
    """int64 [N,3]: the lattice indices with every index a multiple of stride, row-major over the strided lattice."""
    ax = [np.arange(0, n, stride) for n in dims]
    I, J, K = np.meshgrid(*ax, indexing="ij")
    return np.stack([I.reshape(-1), J.reshape(-1), K.reshape(-1)], 1)


def sample_terms(D, S, pose, stride, min_weight=1.0, huber=0.5):
    """What gs_tsdf_register_system computes per sample of one pose (S-world to D-world, float64 [3,4]): {"considered",
    "valid": bool [N], "f": the residual r, "fd": D's value, "fr": S's value times the ratio, "wt": float32 [N], "J":
    float32 [N,6], "q", "pw", "p": float32 [N,3], "idx": int64 [N,3]}.  ("f" is the name tsdf_align_restatement's
    `sample_rows` reads the residual under.)"""
    idx = strided_samples(S["tsdf"].shape, stride)
    min_weight, huber = F(min_weight), F(huber)
    ratio = F(S["trunc"]) / F(D["trunc"])
    m = np.asarray(pose, np.float64).reshape(3, 4).astype(F)
    with np.errstate(all="ignore"):
        ws, fs = S["weight"][idx[:, 0], idx[:, 1], idx[:, 2]], S["tsdf"][idx[:, 0], idx[:, 1], idx[:, 2]]
        fr = fs * ratio
        considered = (ws >= min_weight) & (np.abs(fs) < F(1)) & (np.abs(fr) < F(1))
        p = [F(S["lo"][r]) + idx[:, r].astype(F) * F(S["voxel"]) for r in range(3)]
        q = [(m[r, 0] * p[0] + m[r, 1] * p[1]) + m[r, 2] * p[2] for r in range(3)]
        pw = [q[r] + m[r, 3] for r in range(3)]
        g, a, inside, at = cell(pw, D)
        valid = considered & inside
        at = np.where(valid, at, 0)
        offs = corner_offsets(D["tsdf"].shape)
        for o in offs:
            valid &= D["weight"].reshape(-1)[at + o] >= min_weight
        v000, v001, v010, v011, v100, v101, v110, v111 = (D["tsdf"].reshape(-1)[at + o] for o in offs)
        sx, sy, sz = (g[r] - a[r] for r in range(3))
        z00, z01, z10, z11 = lerp(v000, v001, sz), lerp(v010, v011, sz), lerp(v100, v101, sz), lerp(v110, v111, sz)
        x0, x1 = lerp(z00, z01, sy), lerp(z10, z11, sy)
        f = lerp(x0, x1, sx)
        valid &= np.abs(f) < F(1)
        y00, y01, y10, y11 = lerp(v000, v010, sy), lerp(v001, v011, sy), lerp(v100, v110, sy), lerp(v101, v111, sy)
        n = [x1 - x0, lerp(z01, z11, sx) - lerp(z00, z10, sx), lerp(y01, y11, sx) - lerp(y00, y10, sx)]
        gw = [c / F(D["voxel"]) for c in n]
        J = np.stack([gw[0], gw[1], gw[2], q[1] * gw[2] - q[2] * gw[1], q[2] * gw[0] - q[0] * gw[2],
                      q[0] * gw[1] - q[1] * gw[0]], axis=1)
        r = f - fr
        ar = np.abs(r)
        wt = np.where(ar <= huber, F(1), huber / ar)
    assert J.dtype == F and r.dtype == F and wt.dtype == F
    return {"considered": considered, "valid": valid, "f": r, "fd": f, "fr": fr, "wt": wt, "J": J, "q": np.stack(q, 1),
            "pw": np.stack(pw, 1), "p": np.stack(p, 1), "idx": idx}


def system(D, S, pose, stride, chunk, min_weight=1.0, huber=0.5):
    """gs_tsdf_register_system: float64 [B,32].  pose float64 [B,3,4]."""
    pose = np.asarray(pose, np.float64).reshape(-1, 3, 4)
    out = np.zeros((pose.shape[0], ROW), np.float64)
    for b in range(pose.shape[0]):
        out[b] = AR.chunked_sum(AR.sample_rows(sample_terms(D, S, pose[b], stride, min_weight, huber)), chunk)
    return out


def register(D, S, pose, chunk, levels=AR.DEFAULT_LEVELS, huber=0.5, min_weight=1.0, lam_rel=1e-6, lam_abs=1e-9,
             min_count=64):
    """register_volumes' sequence: per level (stride, iterations) system and gs_tsdf_align_step, then one closing system
    at the last level's stride.  -> (pose [B,3,4], closing rows [B,32], trace [iterations,B,4])."""
    pose = np.array(pose, np.float64).reshape(-1, 3, 4)
    trace = []
    for stride, iters in levels:
        for _ in range(iters):
            out = system(D, S, pose, stride, chunk, min_weight, huber)
            pose, tr = AR.step(out, pose, lam_rel, lam_abs, min_count)
            trace.append(tr)
    closing = system(D, S, pose, levels[-1][0], chunk, min_weight, huber)
    return pose, closing, np.array(trace, np.float64).reshape(len(trace), pose.shape[0], 4)


def merge(D, S, d2s=None, min_weight=1.0, max_weight=64.0, dtype=F):
    """gs_tsdf_merge: a new volume dict, D with S fused in, and "touched": bool [nx,ny,nz], the points that were not
    skipped.  d2s: D-world to S-world, [3,4] (rounded to float32 here as the host does; None: the identity).  Colours are
    fused only when both volumes carry them.  dtype=np.float64 is the same sequence in double on volumes whose arrays are
    double: the analytic checks use it, nothing else does."""
    F = dtype
    if not F(S["trunc"]) >= F(D["trunc"]):
        raise ValueError("merge: trunc_S < trunc_D")
    dims = D["tsdf"].shape
    m = np.concatenate([np.eye(3), np.zeros((3, 1))], 1) if d2s is None else np.asarray(d2s, np.float64).reshape(3, 4)
    m = m.astype(F)
    ratio = F(S["trunc"]) / F(D["trunc"])
    min_weight, max_weight = F(min_weight), F(max_weight)
    idx = strided_samples(dims, 1)
    out = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in D.items()}
    with np.errstate(all="ignore"):
        p = [F(D["lo"][r]) + idx[:, r].astype(F) * F(D["voxel"]) for r in range(3)]
        ps = [((m[r, 0] * p[0] + m[r, 1] * p[1]) + m[r, 2] * p[2]) + m[r, 3] for r in range(3)]
        g, a, inside, at = cell(ps, S, F)
        offs = corner_offsets(S["tsdf"].shape)
        wc = [S["weight"].reshape(-1)[at + o] for o in offs]
        keep = inside.copy()
        for c in wc:
            keep &= c >= min_weight
        sx, sy, sz = (g[r] - a[r] for r in range(3))
        fs = trilinear([S["tsdf"].reshape(-1)[at + o] for o in offs], sx, sy, sz)
        ws = trilinear(wc, sx, sy, sz)
        s = fs * ratio
        keep &= ~(s < F(-1))
        s = np.fmin(F(1), s)                                   # fminf: the number when one side is a NaN
        w0 = D["weight"].reshape(-1)
        w1 = w0 + ws
        tsdf = (D["tsdf"].reshape(-1) * w0 + s * ws) / w1
        out["tsdf"] = np.where(keep, tsdf, D["tsdf"].reshape(-1)).reshape(dims)
        out["weight"] = np.where(keep, np.fmin(w1, max_weight), w0).reshape(dims)
        if "colors" in D and "colors" in S:
            for ch in range(3):
                cs = trilinear([S["colors"][ch].reshape(-1)[at + o] for o in offs], sx, sy, sz)
                cd = D["colors"][ch].reshape(-1)
                out["colors"][ch] = np.where(keep, (cd * w0 + cs * ws) / w1, cd).reshape(dims)
    assert out["tsdf"].dtype == F and out["weight"].dtype == F
    out["touched"] = keep.reshape(dims)
    return out


# ---- the analytic room in a moved frame -------------------------------------------------------------------------------
def room_sdf(points, planes):
    """float64: the room's signed distance (min of the three plane distances, from inside x > px, y > py, z < pz) at
    world points [...,3]."""
    return np.minimum(np.minimum(points[..., 0] - planes[0], points[..., 1] - planes[1]), planes[2] - points[..., 2])


def moved_room(dims, voxel, trunc, T, planes, centre):
    """The room `planes` sampled analytically on a lattice that lives in a frame S with D-world = T S-world (T float64
    [3,4]), centred so that the lattice's middle maps to the D-world point `centre`: (volume dict with weight 1, the
    nearest plane's number per lattice point int64 [nx,ny,nz], the unclipped sdf float64)."""
    T = np.asarray(T, np.float64)
    c_s = T[:, :3].T @ (np.asarray(centre, np.float64) - T[:, 3])
    lo = c_s - 0.5 * voxel * (np.asarray(dims) - 1)
    ax = [lo[a] + voxel * np.arange(dims[a], dtype=np.float64) for a in range(3)]
    P = np.stack(np.meshgrid(*ax, indexing="ij"), -1)
    Pw = P @ T[:, :3].T + T[:, 3]
    dist = np.stack([Pw[..., 0] - planes[0], Pw[..., 1] - planes[1], planes[2] - Pw[..., 2]], -1)
    sdf = dist.min(-1)
    vol = volume(np.clip(sdf / trunc, -1.0, 1.0).astype(F), np.ones(dims, F), lo, voxel, trunc)
    return vol, dist.argmin(-1), sdf


def displaced_transform(T, metres, degrees, rng):
    """`T` (S-world to D-world) moved by `metres` along a random direction and turned by `degrees` about a random axis,
    the step's own convention: o + v, exp(omega) R."""
    return AR.displaced(np.asarray(T, np.float64), metres, degrees, rng)


def inverse(T):
    """The inverse of a rigid [3,4] transform in float64."""
    T = np.asarray(T, np.float64)
    Rt = T[:, :3].T
    return np.concatenate([Rt, -(Rt @ T[:, 3:])], 1)
