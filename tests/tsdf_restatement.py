"""csrc/tsdf.hip restated in NumPy: serial over frames, vectorised over lattice points, one rounding per operation.

The contract (include/goslam_hip.h, gs_tsdf_integrate), per lattice point (i,j,k) and frame, in fp32, no fma:

    p   = lo + float(idx) * voxel                       (per axis)
    pc  = R p + t   as ((r0*px + r1*py) + r2*pz) + t    (per row)
    skip if !(pc.z > 1e-3)
    u = fx * (pc.x / pc.z) + cx ; v = fy * (pc.y / pc.z) + cy
    fu = floorf(u + 0.5f) ; fv likewise ; skip unless 0 <= fu < w and 0 <= fv < h ; iu = (int)fu ; iv = (int)fv
    d = depth[iv,iu] ; skip if !(d > 0) or mask[iv,iu] == 0
    sdf = d - pc.z ; skip if sdf < -trunc
    s = fminf(1.0f, sdf / trunc)
    w1 = w0 + 1.0f
    tsdf = (tsdf * w0 + s) / w1
    if sdf <= trunc: colour = (colour * w0 + images[:,iv,iu]) / w1   (per channel)
    w = fminf(w1, max_weight)

`integrate(..., dtype=np.float64)` is the same sequence in double: the analytic checks use it, nothing else does.
gs_tsdf_vertex_attr: a = floor of every coordinate, b = a plus one along the first axis with t = c - floor(c) > 0;
keep = weight[a] >= min_weight and weight[b] >= min_weight; rgb = colors[a] + t * (colors[b] - colors[a]).
"""
import numpy as np


def new_volume(dims, dtype=np.float32):
    return {"tsdf": np.ones(dims, dtype), "weight": np.zeros(dims, dtype), "colors": np.zeros((3,) + tuple(dims), dtype)}


def lattice_dims(bound, voxel):
    bound = np.asarray(bound, dtype=np.float64)
    return tuple(int(np.ceil((bound[a, 1] - bound[a, 0]) / voxel)) + 1 for a in range(3))


def lattice_axes(dims, lo, voxel, dtype=np.float32):
    """(px [nx,1,1], py [1,ny,1], pz [1,1,nz]): lo + float(idx) * voxel per axis, in `dtype`."""
    T = dtype
    nx, ny, nz = dims
    vx = T(voxel)
    return ((T(lo[0]) + np.arange(nx).astype(T) * vx)[:, None, None], (T(lo[1]) + np.arange(ny).astype(T) * vx)[None, :, None],
            (T(lo[2]) + np.arange(nz).astype(T) * vx)[None, None, :])


def frame_geometry(f, depth, w2c, intr, px, py, pz, trunc, mask, dtype=np.float32):
    """The contract's steps up to the sdf < -trunc skip for frame f of depth ([K,H,W], already in `dtype`): (sel flat
    indices of the lattice points that are updated, sdf, iu, iv).  tsdf_live_restatement.accumulate walks it too."""
    T = dtype
    fx, fy, cx, cy = (T(v) for v in intr)
    tr, half, near = T(trunc), T(0.5), T(1e-3)
    _, H, W = depth.shape
    m = np.asarray(w2c[f]).astype(T)
    z = (((m[2, 0] * px + m[2, 1] * py) + m[2, 2] * pz) + m[2, 3]).reshape(-1)
    x = (((m[0, 0] * px + m[0, 1] * py) + m[0, 2] * pz) + m[0, 3]).reshape(-1)
    y = (((m[1, 0] * px + m[1, 1] * py) + m[1, 2] * pz) + m[1, 3]).reshape(-1)
    sel = np.nonzero(z > near)[0]
    x, y, z = x[sel], y[sel], z[sel]
    u = fx * (x / z) + cx
    v = fy * (y / z) + cy
    fu, fv = np.floor(u + half), np.floor(v + half)
    ok = (fu >= 0) & (fu < T(W)) & (fv >= 0) & (fv < T(H))
    sel, z = sel[ok], z[ok]
    iu, iv = fu[ok].astype(np.int64), fv[ok].astype(np.int64)
    d = depth[f, iv, iu]
    ok = d > 0
    if mask is not None:
        ok &= ~(np.asarray(mask[f]).astype(T)[iv, iu] == 0)
    sel, z, d, iu, iv = sel[ok], z[ok], d[ok], iu[ok], iv[ok]
    sdf = d - z
    ok = ~(sdf < -tr)
    return sel[ok], sdf[ok], iu[ok], iv[ok]


def integrate(vol, depth, w2c, intr, lo, voxel, trunc, max_weight=64.0, images=None, mask=None, dtype=np.float32):
    """In place on vol (new_volume's dict).  depth [K,H,W], w2c [K,3,4], images [K,3,H,W] or None, mask [K,H,W] or None;
    every input is first rounded to `dtype`."""
    T = dtype
    tr, mw, one = T(trunc), T(max_weight), T(1.0)
    px, py, pz = lattice_axes(vol["tsdf"].shape, lo, voxel, T)
    depth = np.asarray(depth).astype(T)
    K = depth.shape[0]
    tsdf, weight = vol["tsdf"].reshape(-1), vol["weight"].reshape(-1)
    colors = vol["colors"].reshape(3, -1)
    assert tsdf.dtype == T and np.shares_memory(tsdf, vol["tsdf"])
    with np.errstate(all="ignore"):
        for f in range(K):
            sel, sdf, iu, iv = frame_geometry(f, depth, w2c, intr, px, py, pz, trunc, mask, T)
            s = np.minimum(one, sdf / tr)
            w0 = weight[sel]
            w1 = w0 + one
            tsdf[sel] = (tsdf[sel] * w0 + s) / w1
            if images is not None:
                c = sdf <= tr
                img = np.asarray(images[f]).astype(T)
                for ch in range(3):
                    colors[ch, sel[c]] = (colors[ch, sel[c]] * w0[c] + img[ch, iv[c], iu[c]]) / w1[c]
            weight[sel] = np.minimum(w1, mw)
    return vol


def vertex_attr(verts, weight, colors, min_weight):
    """-> (keep bool [V], rgb float32 [V,3]) for float32 vertices in index space."""
    verts = np.ascontiguousarray(verts, dtype=np.float32)
    V = len(verts)
    fl = np.floor(verts)
    fr = verts - fl
    dims = np.array(weight.shape)
    a = np.clip(np.nan_to_num(fl, nan=0.0), 0, dims - 1).astype(np.int64)
    b = a.copy()
    t = np.zeros(V, np.float32)
    found = np.zeros(V, bool)
    for d in range(3):
        hit = ~found & (fr[:, d] > 0)
        t[hit] = fr[hit, d]
        b[hit, d] = np.minimum(a[hit, d] + 1, dims[d] - 1)
        found |= hit
    wa, wb = weight[a[:, 0], a[:, 1], a[:, 2]], weight[b[:, 0], b[:, 1], b[:, 2]]
    keep = (wa >= np.float32(min_weight)) & (wb >= np.float32(min_weight))
    ca = colors[:, a[:, 0], a[:, 1], a[:, 2]].T.astype(np.float32)
    cb = colors[:, b[:, 0], b[:, 1], b[:, 2]].T.astype(np.float32)
    rgb = ca + t[:, None] * (cb - ca)
    return keep, rgb.astype(np.float32)


def extract_mesh(vol, lo, voxel, min_weight=1.0):
    """TSDFVolume.extract_mesh's steps on a restated lattice: mesh_restatement's marching cubes over -tsdf, vertex_attr,
    faces whose three vertices are kept, unreferenced vertices dropped, v * voxel + lo in float64, colours as
    pointcloud.ply_colors makes them -> (vertices float64 [V,3], faces int64 [F,3], colours uint8 [V,3])."""
    import mesh_restatement as MR
    verts, faces = MR.marching_cubes(-vol["tsdf"].astype(np.float32), 0.0)
    if len(faces) == 0:
        return np.zeros((0, 3)), np.zeros((0, 3), np.int64), np.zeros((0, 3), np.uint8)
    keep, rgb = vertex_attr(verts, vol["weight"].astype(np.float32), vol["colors"].astype(np.float32), min_weight)
    faces = faces[keep[faces].all(axis=1)].astype(np.int64)
    used = np.zeros(len(verts), bool)
    used[faces.reshape(-1)] = True
    remap = np.cumsum(used) - 1
    colours = (np.clip(rgb.astype(np.float64), 0.0, 1.0) * 255.0).astype(np.uint8)
    return (verts[used].astype(np.float64) * float(voxel) + np.asarray(lo, np.float64)[None, :],
            remap[faces].reshape(-1, 3), colours[used])


# ---- the fronto-parallel scene of the analytic checks: a plane z = c seen by three translated cameras, no rotation --
PLANE_INTR = (61.3, 60.7, 31.37, 23.61)
PLANE_HW = (48, 64)
PLANE_CAMS = np.array([[0.013, -0.021, 0.0], [0.317, 0.113, 0.0], [-0.263, -0.157, 0.1]])     # camera centres
PLANE_BOUND = np.array([[-1.0, 1.0], [-0.75, 0.75], [0.0, 2.5]])
PLANE_VOXEL = 0.05


def plane_scene(c):
    """(depth f32 [3,H,W], w2c f32 [3,3,4]) of the plane z = c: a camera at centre q sees the constant depth c - q.z."""
    H, W = PLANE_HW
    depth = np.stack([np.full((H, W), c - q[2]) for q in PLANE_CAMS]).astype(np.float32)
    w2c = np.zeros((3, 3, 4), np.float32)
    w2c[:, :, :3] = np.eye(3)
    w2c[:, :, 3] = -PLANE_CAMS
    return depth, w2c


def plane_projection_counts(dims, margin=1e-4):
    """In float64, straight from the geometry: per lattice point of the plane scene, how many cameras hold its rounded
    projection in their image (in front of the near plane), and whether some camera's u + 0.5 or v + 0.5 lies within
    `margin` of an integer (fp32 may then round the pixel the other way)."""
    fx, fy, cx, cy = PLANE_INTR
    H, W = PLANE_HW
    g = np.meshgrid(*[PLANE_BOUND[a, 0] + np.arange(dims[a]) * PLANE_VOXEL for a in range(3)], indexing="ij")
    count = np.zeros(dims, np.int64)
    shaky = np.zeros(dims, bool)
    for q in PLANE_CAMS:
        zc = g[2] - q[2]
        front = zc > 1e-3
        with np.errstate(all="ignore"):
            u = fx * (g[0] - q[0]) / zc + cx + 0.5
            v = fy * (g[1] - q[1]) / zc + cy + 0.5
            inside = front & (np.floor(u) >= 0) & (np.floor(u) < W) & (np.floor(v) >= 0) & (np.floor(v) < H)
            shaky |= front & ((np.abs(u - np.round(u)) < margin) | (np.abs(v - np.round(v)) < margin))
        count += inside
        shaky |= np.abs(zc - 1e-3) < 1e-6
    return count, shaky
