"""csrc/esdf.hip restated in NumPy: serial over the offsets of a window, vectorised over lattice points; every fp32
step is an explicit np.float32 operation.

The contract (include/goslam_hip.h, gs_esdf_*):

    state = 0 when !(weight >= min_weight), else 2 when tsdf < 0, else 1
    site  : state != 0 and a 6-neighbour inside the lattice with state != 0 and another state
    d2    : start 0 at sites, INF elsewhere; along z, then y, then x
              out[i] = min over |k| <= R, 0 <= i + k < n of in[i + k] + k * k
            then every value > R * R becomes FAR
    dist  = sign * (voxel * sqrtf(float(d2))), FAR -> sign * (voxel * float(R)); sign = -1 where state == 2

`window_min` is that minimum written out plainly, without the kernels' early exit; `early_exit_min` is the kernels' loop
(best = in[i]; for k = 1; k <= R and k * k < best: ...), kept here so that the CPU tests can hold the two together.
`query` and `occupancy_slice` restate gs_esdf_query and gs_esdf_slice.
"""
import numpy as np

INF = 0x3fffffff
FAR = 0x7fffffff
F = np.float32


def states(tsdf, weight, min_weight=1.0):
    tsdf, weight = np.asarray(tsdf, F), np.asarray(weight, F)
    with np.errstate(invalid="ignore"):
        known = weight >= F(min_weight)
        solid = tsdf < F(0.0)
    return np.where(known, np.where(solid, 2, 1), 0).astype(np.uint8)


def site_mask(state):
    site = np.zeros(state.shape, bool)
    for axis in range(3):
        a = [slice(None)] * 3
        b = [slice(None)] * 3
        a[axis], b[axis] = slice(0, -1), slice(1, None)
        a, b = tuple(a), tuple(b)
        change = (state[a] != 0) & (state[b] != 0) & (state[a] != state[b])
        site[a] |= change
        site[b] |= change
    return site


def _shifted(f, axis, k):
    """(view of out positions i, view of in positions i + k) along axis, both inside the line."""
    n = f.shape[axis]
    dst, src = [slice(None)] * 3, [slice(None)] * 3
    if k >= 0:
        dst[axis], src[axis] = slice(0, n - k), slice(k, n)
    else:
        dst[axis], src[axis] = slice(-k, n), slice(0, n + k)
    return tuple(dst), tuple(src)


def window_min(f, axis, R):
    """The plain windowed minimum of one pass.  Offsets with |k| >= n have no term inside the line."""
    f = np.asarray(f, np.int64)
    out = f.copy()
    for k in range(1, min(int(R), f.shape[axis] - 1) + 1):
        for s in (k, -k):
            dst, src = _shifted(f, axis, s)
            out[dst] = np.minimum(out[dst], f[src] + k * k)
    return out


def early_exit_min(f, axis, R):
    """The kernels' loop, per point: a point leaves the loop at the first k with k * k >= best and never comes back
    (best only falls, k * k only grows)."""
    f = np.asarray(f, np.int64)
    best = f.copy()
    going = np.ones(f.shape, bool)
    for k in range(1, min(int(R), f.shape[axis] - 1) + 1):
        going &= k * k < best
        if not going.any():
            break
        for s in (k, -k):
            dst, src = _shifted(f, axis, s)
            cand = np.minimum(best[dst], f[src] + k * k)
            best[dst] = np.where(going[dst], cand, best[dst])
    return best


def squared_distance(site, R, line_min=window_min):
    R = int(R)
    f = np.where(site, 0, INF).astype(np.int64)
    for axis in (2, 1, 0):
        f = line_min(f, axis, R)
    assert f.max() <= INF
    return np.where(f > R * R, FAR, f).astype(np.int32)


def distance(d2, state, R, voxel):
    root = np.sqrt(np.where(d2 == FAR, 0, d2).astype(F))               # exact conversion: d2 < 2^24
    assert root.dtype == F
    mag = F(voxel) * np.where(d2 == FAR, F(int(R)), root).astype(F)
    sign = np.where(state == 2, F(-1.0), F(1.0)).astype(F)
    out = sign * mag
    assert out.dtype == F
    return out


def build(tsdf, weight, R, voxel, min_weight=1.0):
    """-> {"state" u8, "site" bool, "d2" i32, "dist" f32}."""
    state = states(tsdf, weight, min_weight)
    site = site_mask(state)
    d2 = squared_distance(site, R)
    return {"state": state, "site": site, "d2": d2, "dist": distance(d2, state, R, voxel)}


def _lerp(p, q, s):
    return p + s * (q - p)


def query(dist, state, lo, voxel, points):
    """-> dist f32 [N], grad f32 [N,3], valid bool [N], known bool [N]."""
    dist, points = np.asarray(dist, F), np.asarray(points, F).reshape(-1, 3)
    N = len(points)
    dims = dist.shape
    vx = F(voxel)
    with np.errstate(all="ignore"):
        g = np.stack([(points[:, a] - F(lo[a])) / vx for a in range(3)], 1)
        fl = np.floor(g)
        valid = np.ones(N, bool)
        for a in range(3):
            valid &= (fl[:, a] >= F(0.0)) & (fl[:, a] < F(dims[a] - 1))
    out_d, out_g, known = np.zeros(N, F), np.zeros((N, 3), F), np.zeros(N, bool)
    sel = np.nonzero(valid)[0]
    a = fl[sel].astype(np.int64)
    s = (g[sel] - fl[sel]).astype(F)
    sx, sy, sz = s[:, 0], s[:, 1], s[:, 2]
    v = {}
    k = np.ones(len(sel), bool)
    for X in (0, 1):
        for Y in (0, 1):
            for Z in (0, 1):
                at = (a[:, 0] + X, a[:, 1] + Y, a[:, 2] + Z)
                v[X, Y, Z] = dist[at]
                k &= state[at] != 0
    z = {(X, Y): _lerp(v[X, Y, 0], v[X, Y, 1], sz) for X in (0, 1) for Y in (0, 1)}
    y = {(X, Z): _lerp(v[X, 0, Z], v[X, 1, Z], sy) for X in (0, 1) for Z in (0, 1)}
    x0, x1 = _lerp(z[0, 0], z[0, 1], sy), _lerp(z[1, 0], z[1, 1], sy)
    out_d[sel] = _lerp(x0, x1, sx)
    out_g[sel, 0] = (x1 - x0) / vx
    out_g[sel, 1] = (_lerp(z[0, 1], z[1, 1], sx) - _lerp(z[0, 0], z[1, 0], sx)) / vx
    out_g[sel, 2] = (_lerp(y[0, 1], y[1, 1], sx) - _lerp(y[0, 0], y[1, 0], sx)) / vx
    known[sel] = k
    assert out_d.dtype == F and out_g.dtype == F and x0.dtype == F
    return out_d, out_g, valid, known


def occupancy_slice(state, d2, dist, up_axis, k0, k1, occ_d2, min_known):
    """-> cells u8 [n_u,n_v], clearance f32 [n_u,n_v]; the layers are visited in increasing order."""
    st, dd, di = (np.moveaxis(np.asarray(t), up_axis, 0) for t in (state, d2, dist))      # [n_a, n_u, n_v]
    occupied = np.zeros(st.shape[1:], bool)
    n_known = np.zeros(st.shape[1:], np.int64)
    c = di[k0].astype(F).copy()
    for k in range(k0, k1 + 1):
        occupied |= (st[k] == 2) | (dd[k] <= occ_d2)
        n_known += st[k] != 0
        c = np.where(di[k] < c, di[k], c)
    cells = np.where(occupied, 0, np.where(n_known >= min_known, 254, 205)).astype(np.uint8)
    return cells, c.astype(F)
