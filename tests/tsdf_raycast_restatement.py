"""csrc/tsdf_raycast.hip restated in NumPy: serial over frames and over the steps of the march, vectorised over the
pixels of a frame, one rounding per operation.

The contract (include/goslam_hip.h, gs_tsdf_raycast), per pixel (iu, iv), in fp32, no fma; a MISS writes depth = 0,
normal = 0, colour = 0:

    dx = (float(iu) - cx) / fx ; dy = (float(iv) - cy) / fy
    dw = (r0 * dx + r1 * dy) + r2                                     (per row of c2w)
    og = (o - lo) / voxel ; dg = dw / voxel                           (per axis; index space, g(t) = og + t * dg)
    MISS unless og and dg are finite on every axis
    dt = (step_voxels * voxel) / sqrtf((dw.x * dw.x + dw.y * dw.y) + dw.z * dw.z) ; MISS unless 0 < dt < inf
    t0 = near ; t1 = far ; per axis with top = float(n - 1):
      dg == 0: MISS unless 0 <= og <= top                             (the axis constrains nothing otherwise)
      else   : ta = (0 - og) / dg ; tb = (top - og) / dg ; t0 = max(t0, min(ta, tb)) ; t1 = min(t1, max(ta, tb))
    for i = 0 .. GS_TSDF_RAY_STEPS: t_i = t0 + float(i) * dt ; stop (MISS) unless t_i < t1
      sample(t): g = og + t * dg (per axis) ; a = floorf(g) ; valid iff 0 <= a < top on every axis (compared as
        floats) and weight >= min_weight at all eight corners a + {0,1}^3 ; fr = g - a ;
        value = trilinear tsdf, lerp(p, q, s) = p + s * (q - p) along z (four), then y (two), then x (one).
      HIT at the first i >= 1 with sample(t_{i-1}) and sample(t_i) valid, f_{i-1} >= 0 and f_i < 0:
        depth = t* = t_{i-1} + dt * (f_{i-1} / (f_{i-1} - f_i)).
    GS_TSDF_RAY_STEPS = ceil((nx + ny + nz) / step_voxels) + 2, in double from the float step_voxels.
    at the hit: the cell of g(t*), valid as above or else MISS (depth too).  With v[x][y][z] its corners and
      (sx, sy, sz) = fr, the gradient of the trilinear interpolant, every lerp as above:
        n.x = yx(1) - yx(0), yx(b) = lerp over y of the two z-lerps of face x = b        (lerps z, then y)
        n.y = zx(1) - zx(0), zx(b) = lerp over x of the two z-lerps of face y = b        (lerps z, then x)
        n.z = yx'(1) - yx'(0), yx'(b) = lerp over x of the two y-lerps of face z = b     (lerps y, then x)
      len = sqrtf((n.x * n.x + n.y * n.y) + n.z * n.z) ; normal = n / len per component, 0 where !(len > 0)
      colour = trilinear colors per channel, lerps z, y, x.

`raycast(..., flags=None)` is that march with no shortcut.  With `flags` (brick_flags' bytes) it is the kernel's skip,
restated: a sample whose cell lies in an unflagged brick is not evaluated when reached as t_i, and is evaluated when a
later sample needs it as t_{i-1}.  gs_tsdf_brick_flags: byte (i,j,k) of [bx,by,bz], b = ceil((n - 1) / 8), is 1 if
tsdf < 0 at any lattice point of [8i, min(8i + 8, nx - 1)] x [8j, ..] x [8k, ..], else 0.
`raycast(..., dtype=np.float64)` is the same sequence in double: the analytic checks use it, nothing else does.
"""
import math

import numpy as np

BRICK = 8


def max_steps(dims, step):
    return int(math.ceil(float(sum(dims)) / float(np.float32(step)))) + 2


def brick_dims(dims):
    return tuple((n - 1 + BRICK - 1) // BRICK for n in dims)


def brick_flags(tsdf):
    tsdf = np.asarray(tsdf)
    bd = brick_dims(tsdf.shape)
    flags = np.zeros(bd, np.uint8)
    for i in range(bd[0]):
        for j in range(bd[1]):
            for k in range(bd[2]):
                block = tsdf[8 * i:8 * i + 9, 8 * j:8 * j + 9, 8 * k:8 * k + 9]       # slices clamp at the lattice's end
                flags[i, j, k] = 1 if (block < 0).any() else 0
    return flags


def _lerp(p, q, s):
    return p + s * (q - p)


def _cell(g, dims, T):
    """g: three arrays -> (in bounds, integer corner (three arrays, 0 where out), fractions)."""
    a = [np.floor(c) for c in g]
    ok = np.ones(g[0].shape, bool)
    for c, n in zip(a, dims):
        ok &= (c >= 0) & (c < T(n - 1))
    idx = [np.where(ok, c, 0).astype(np.int64) for c in a]
    return ok, idx, [c - f for c, f in zip(g, a)]


def _corners(arr, idx):
    """v[bx][by][bz] of the cells at idx"""
    return [[[arr[idx[0] + bx, idx[1] + by, idx[2] + bz] for bz in (0, 1)] for by in (0, 1)] for bx in (0, 1)]


def _seen(weight, idx, min_weight):
    w = _corners(weight, idx)
    ok = np.ones(idx[0].shape, bool)
    for bx in (0, 1):
        for by in (0, 1):
            for bz in (0, 1):
                ok &= w[bx][by][bz] >= min_weight
    return ok


def _trilinear(v, s):
    c = [[_lerp(v[bx][by][0], v[bx][by][1], s[2]) for by in (0, 1)] for bx in (0, 1)]
    return _lerp(_lerp(c[0][0], c[0][1], s[1]), _lerp(c[1][0], c[1][1], s[1]), s[0])


def _sample(vol, g, dims, min_weight, T):
    """sample(t) at the points g -> (valid, value; 0 where invalid)"""
    ok, idx, s = _cell(g, dims, T)
    ok = ok & _seen(vol["weight"], idx, min_weight)
    f = _trilinear(_corners(vol["tsdf"], idx), s)
    return ok, np.where(ok, f, T(0))


def raycast(vol, c2w, intr, size, lo, voxel, near=0.0, far=np.inf, step=0.5, min_weight=1.0, color=True, flags=None,
            dtype=np.float32, stats=None):
    """vol: tsdf_restatement.new_volume's dict; c2w [K,3,4]; size (H, W).  -> {"depth" [K,H,W], "normal" [K,H,W,3],
    "color" [K,H,W,3] or None} in `dtype`; every input is first rounded to `dtype`.  `stats`, a dict, receives
    "samples" (the t_i reached inside [t0, t1)) and "evaluated" (the sample() calls made)."""
    T = dtype
    vol = {k: np.asarray(v).astype(T) for k, v in vol.items()}
    dims = vol["tsdf"].shape
    H, W = size
    fx, fy, cx, cy = (T(v) for v in intr)
    vx, mw, near, far = T(voxel), T(min_weight), T(near), T(far)
    c2w = np.asarray(c2w).astype(T)
    K = len(c2w)
    nmax = max_steps(dims, step)
    iv, iu = (a.reshape(-1) for a in np.meshgrid(np.arange(H), np.arange(W), indexing="ij"))
    depth = np.zeros((K, H * W), T)
    normal = np.zeros((K, H * W, 3), T)
    colour = np.zeros((K, H * W, 3), T) if color else None
    n_samples = n_eval = 0
    with np.errstate(all="ignore"):
        dx, dy = (iu.astype(T) - cx) / fx, (iv.astype(T) - cy) / fy
        for k in range(K):
            m = c2w[k]
            dw = [(m[r, 0] * dx + m[r, 1] * dy) + m[r, 2] for r in range(3)]
            og = [np.full(dx.shape, (m[r, 3] - T(lo[r])) / vx, T) for r in range(3)]
            dg = [d / vx for d in dw]
            alive = np.ones(dx.shape, bool)
            for r in range(3):
                alive &= np.isfinite(og[r]) & np.isfinite(dg[r])
            dt = (T(step) * vx) / np.sqrt((dw[0] * dw[0] + dw[1] * dw[1]) + dw[2] * dw[2])
            alive &= (dt > 0) & (dt < np.inf)
            t0, t1 = np.full(dx.shape, near, T), np.full(dx.shape, far, T)
            for r in range(3):
                top = T(dims[r] - 1)
                zero = dg[r] == 0
                alive &= ~zero | ((og[r] >= 0) & (og[r] <= top))
                ta, tb = (T(0) - og[r]) / dg[r], (top - og[r]) / dg[r]
                a, b = np.where(ta < tb, ta, tb), np.where(ta < tb, tb, ta)
                t0 = np.where(~zero & (a > t0), a, t0)
                t1 = np.where(~zero & (b < t1), b, t1)
            px = np.nonzero(alive)[0]                      # pixels still marching
            st = {"og": [c[px] for c in og], "dg": [c[px] for c in dg], "dt": dt[px], "t0": t0[px], "t1": t1[px],
                  "known": np.zeros(len(px), bool), "valid": np.zeros(len(px), bool), "f": np.zeros(len(px), T)}

            def keep(sel):
                for key, val in st.items():
                    st[key] = [c[sel] for c in val] if isinstance(val, list) else val[sel]

            def point(t):
                return [o + t * d for o, d in zip(st["og"], st["dg"])]

            hit_px, hit_t = [], []
            for i in range(nmax + 1):
                t = st["t0"] + T(i) * st["dt"]
                go = t < st["t1"]
                px, t = px[go], t[go]
                keep(go)
                if len(px) == 0:
                    break
                n_samples += len(px)
                g = point(t)
                if flags is None:
                    valid, f = _sample(vol, g, dims, mw, T)
                    known = np.ones(len(px), bool)
                    n_eval += len(px)
                else:
                    inb, idx, _ = _cell(g, dims, T)
                    known = ~(inb & (flags[idx[0] >> 3, idx[1] >> 3, idx[2] >> 3] == 0))
                    valid, f = _sample(vol, g, dims, mw, T)
                    valid, f = valid & known, np.where(known, f, T(0))       # a skipped sample is not looked at
                    n_eval += int(known.sum())
                if i >= 1:
                    tp = st["t0"] + T(i - 1) * st["dt"]
                    cand = known & valid & (f < 0)
                    need = cand & ~st["known"]             # the sample before was skipped: evaluate it now
                    if need.any():
                        pv, pf = _sample(vol, point(tp), dims, mw, T)
                        st["valid"], st["f"] = np.where(need, pv, st["valid"]), np.where(need, pf, st["f"])
                        n_eval += int(need.sum())
                    hit = cand & st["valid"] & (st["f"] >= 0)
                    if hit.any():
                        fp = st["f"]
                        hit_px.append(px[hit])
                        hit_t.append((tp + st["dt"] * (fp / (fp - f)))[hit])
                else:
                    hit = np.zeros(len(px), bool)
                st["known"], st["valid"], st["f"] = known, valid, f
                px = px[~hit]
                keep(~hit)
            if not hit_px:
                continue
            # the hits: normal and colour in the cell of g(t*)
            hp, ts = np.concatenate(hit_px), np.concatenate(hit_t)
            g = [og[r][hp] + ts * dg[r][hp] for r in range(3)]
            ok, idx, s = _cell(g, dims, T)
            ok &= _seen(vol["weight"], idx, mw)
            v = _corners(vol["tsdf"], idx)
            z = [[_lerp(v[bx][by][0], v[bx][by][1], s[2]) for by in (0, 1)] for bx in (0, 1)]       # z[x][y]
            y = [[_lerp(v[bx][0][bz], v[bx][1][bz], s[1]) for bz in (0, 1)] for bx in (0, 1)]       # y[x][z]
            nx = _lerp(z[1][0], z[1][1], s[1]) - _lerp(z[0][0], z[0][1], s[1])
            ny = _lerp(z[0][1], z[1][1], s[0]) - _lerp(z[0][0], z[1][0], s[0])
            nz = _lerp(y[0][1], y[1][1], s[0]) - _lerp(y[0][0], y[1][0], s[0])
            length = np.sqrt((nx * nx + ny * ny) + nz * nz)
            pos = ok & (length > 0)
            depth[k, hp] = np.where(ok, ts, T(0))
            for c, comp in enumerate((nx, ny, nz)):
                normal[k, hp, c] = np.where(pos, comp / length, T(0))
            if color:
                for c in range(3):
                    colour[k, hp, c] = np.where(ok, _trilinear(_corners(vol["colors"][c], idx), s), T(0))
    if stats is not None:
        stats["samples"], stats["evaluated"] = n_samples, n_eval
    return {"depth": depth.reshape(K, H, W), "normal": normal.reshape(K, H, W, 3),
            "color": colour.reshape(K, H, W, 3) if color else None}
