"""csrc/tsdf_live.hip restated in NumPy, straight from include/goslam_hip.h (gs_tsdf_accumulate, gs_tsdf_resolve,
gs_tsdf_frame_change): serial over frames, vectorised over lattice points, fp32 with one rounding per operation.

accumulate, per lattice point and frame: gs_tsdf_integrate's geometry (tsdf_restatement.frame_geometry, the function
tsdf_restatement.integrate walks) and s = fminf(1, sdf / trunc), then in int32

    q = (int)rintf(s * 16384.0f) ; sum_s += sign * q ; count += sign
    if images and sdf <= trunc: c = (int)rintf(fminf(fmaxf(img, 0), 1) * 255.0f) per channel ; sum_rgb += sign * c ;
                                count_rgb += sign

resolve: weight = (float)max(count, 0) ; tsdf = count > 0 ? (float)((double)sum_s / ((double)count * 16384.0)) : 1 ;
colors = count_rgb > 0 ? (float)((double)sum_rgb / ((double)count_rgb * 255.0)) : 0.
frame_change: the four numbers per frame, the sums in the header's order (thread t of 256 takes pixels t, t + 256, ...;
a wave's butterfly v += v[lane ^ m], m = 32 .. 1; the four waves as ((w0 + w1) + w2) + w3).
`observations` returns the unquantised s and clamped colours per (frame, point) for the closed-form checks.
"""
import numpy as np

from tsdf_restatement import frame_geometry, lattice_axes

Q = 16384.0


def new_state(dims, color=True):
    z = lambda *s: np.zeros(s, np.int32)                    # noqa: E731
    return {"sum_s": z(*dims), "count": z(*dims), "sum_rgb": z(3, *dims) if color else None,
            "count_rgb": z(*dims) if color else None}


def accumulate(state, depth, w2c, intr, lo, voxel, trunc, images=None, mask=None, sign=1, observations=None):
    """In place on `state` (new_state's dict).  depth [K,H,W], w2c [K,3,4], images [K,3,H,W] or None, mask [K,H,W] or
    None, sign a scalar or [K] integers.  With a list `observations`, appends per frame (sel, s float32, colour sel,
    clamped colours float32 [3,n]) -- the values before quantisation."""
    T = np.float32
    dims = state["sum_s"].shape
    px, py, pz = lattice_axes(dims, lo, voxel)
    depth = np.asarray(depth).astype(T)
    K = depth.shape[0]
    signs = np.broadcast_to(np.asarray(sign, np.int32), (K,))
    sum_s, count = state["sum_s"].reshape(-1), state["count"].reshape(-1)
    assert np.shares_memory(sum_s, state["sum_s"]) and sum_s.dtype == np.int32
    tr, one = T(trunc), T(1.0)
    with np.errstate(all="ignore"):
        for f in range(K):
            sel, sdf, iu, iv = frame_geometry(f, depth, w2c, intr, px, py, pz, trunc, mask)
            s = np.fmin(one, sdf / tr)
            q = np.rint(s * T(Q)).astype(np.int32)
            sum_s[sel] += signs[f] * q
            count[sel] += signs[f]
            obs = [sel, s, None, None]
            if images is not None:
                sum_rgb, count_rgb = state["sum_rgb"].reshape(3, -1), state["count_rgb"].reshape(-1)
                c = sdf <= tr
                img = np.asarray(images[f]).astype(T)[:, iv[c], iu[c]]
                clamped = np.fmin(np.fmax(img, T(0.0)), one)
                sum_rgb[:, sel[c]] += signs[f] * np.rint(clamped * T(255.0)).astype(np.int32)
                count_rgb[sel[c]] += signs[f]
                obs[2:] = [sel[c], clamped]
            if observations is not None:
                observations.append(tuple(obs))
    return state


def resolve(state):
    """-> {"tsdf", "weight" float32 [nx,ny,nz], "colors" float32 [3,nx,ny,nz] or None}."""
    count = state["count"]
    with np.errstate(all="ignore"):
        tsdf = np.where(count > 0, (state["sum_s"].astype(np.float64) / (count.astype(np.float64) * Q)).astype(np.float32),
                        np.float32(1.0))
        colors = None
        if state["sum_rgb"] is not None:
            cc = state["count_rgb"][None]
            colors = np.where(cc > 0, (state["sum_rgb"].astype(np.float64) / (cc.astype(np.float64) * 255.0))
                              .astype(np.float32), np.float32(0.0)).astype(np.float32)
    return {"tsdf": tsdf.astype(np.float32), "weight": np.maximum(count, 0).astype(np.float32), "colors": colors}


def pose_points(m, ref):
    """(c, p) float64 [3] of a float32 [3,4] matrix: c = -R^T t, p = R^T (ref e_z - t), each component as (a + b) + c."""
    m = np.asarray(m, np.float32).astype(np.float64)
    t = m[:, 3]
    c, p = np.zeros(3), np.zeros(3)
    for j in range(3):
        r = m[:, j]
        c[j] = -((r[0] * t[0] + r[1] * t[1]) + r[2] * t[2])
        p[j] = (r[0] * (-t[0]) + r[1] * (-t[1])) + r[2] * (np.float64(ref) - t[2])
    return c, p


def _dist(a, b):
    d = a - b
    return np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])


def _ordered_sum(values):
    """The kernel's order over per-pixel float64 values (0 where a pixel does not count)."""
    n = len(values)
    rows = -(-n // 256)
    v = np.zeros(rows * 256, np.float64)
    v[:n] = values
    part = np.zeros(256, np.float64)
    for r in v.reshape(rows, 256):                          # thread t: pixels t, t + 256, ... in increasing order
        part = part + r
    lane = np.arange(256)
    for m in (32, 16, 8, 4, 2, 1):
        part = part + part[lane ^ m]                        # stays within a wave: m < 64
    w = part[::64]
    return ((w[0] + w[1]) + w[2]) + w[3]


def frame_change(old_depth, cur_depth, w2c_old, w2c_new, ref_depth):
    """-> float64 [k,4]."""
    old_depth, cur_depth = np.asarray(old_depth, np.float32), np.asarray(cur_depth, np.float32)
    k = old_depth.shape[0]
    out = np.zeros((k, 4), np.float64)
    ref = np.float64(np.float32(ref_depth))
    for f in range(k):
        o, c = old_depth[f].reshape(-1), cur_depth[f].reshape(-1)
        both = (o > 0) & (c > 0)
        with np.errstate(all="ignore"):
            diff = np.where(both, np.abs(c - o).astype(np.float64), 0.0)
        out[f, 0] = _ordered_sum(both.astype(np.float64))
        out[f, 1] = _ordered_sum(diff)
        c0, p0 = pose_points(w2c_old[f], ref)
        c1, p1 = pose_points(w2c_new[f], ref)
        out[f, 2], out[f, 3] = _dist(c1, c0), _dist(p1, p0)
    return out
