"""CPU restatements of the mesh-culling contracts of include/goslam_neus.h (gs_mesh_depth, gs_mesh_visibility,
gs_face_components, gs_face_component_areas, the OBB behind gs_hull_*) and of Mesher.cull_mesh's composition, written
from those contracts in NumPy / SciPy / torch-CPU: what go_slam_amd.neus.mesher must agree with."""
import numpy as np
import torch
import torch.nn.functional as F

ZNEAR = 0.001


def mesh_depth(verts, faces, c2w_list, H, W, fx, fy, cx, cy, far=20.0, znear=ZNEAR, edge_tol=1e-3):
    """float64 depth maps [K,H,W] (0 = no hit) and an `ambiguous` bool [K,H,W]: pixel centres within edge_tol pixels of a
    projected edge line of a face whose pixel range contains them, or whose hit lies within 1e-9 relative of znear / far.
    Per pixel centre (c + 0.5, r + 0.5): the nearest z >= znear, <= far at which the ray meets a face (inclusive edges)."""
    verts = np.asarray(verts, np.float64)
    faces = np.asarray(faces, np.int64)
    c2w_list = np.asarray(c2w_list, np.float64).reshape(-1, 4, 4)
    K = len(c2w_list)
    depth = np.full((K, H, W), np.inf)
    amb = np.zeros((K, H, W), bool)
    uu = (np.arange(W) + 0.5 - cx) / fx
    vv = (np.arange(H) + 0.5 - cy) / fy
    for k in range(K):
        w2c = np.linalg.inv(c2w_list[k])
        P = verts @ w2c[:3, :3].T + w2c[:3, 3]
        for f in faces:
            if len(set(f.tolist())) < 3:
                continue
            T = P[f]
            if not np.isfinite(T).all() or T[:, 2].max() < znear or T[:, 2].min() > far:
                continue
            n = np.cross(T[1] - T[0], T[2] - T[0])
            if not n.any():
                continue
            # screen bounds of the part with z >= znear
            pts = [T[i] for i in range(3) if T[i, 2] >= znear]
            for i in range(3):
                a, b = T[i], T[(i + 1) % 3]
                if (a[2] < znear) != (b[2] < znear):
                    t = (znear - a[2]) / (b[2] - a[2])
                    pts.append(a + t * (b - a))
            pts = np.array(pts)
            u = fx * pts[:, 0] / pts[:, 2] + cx
            v = fy * pts[:, 1] / pts[:, 2] + cy
            c0, c1 = max(int(np.ceil(u.min() - 0.5)) - 1, 0), min(int(np.floor(u.max() - 0.5)) + 1, W - 1)
            r0, r1 = max(int(np.ceil(v.min() - 0.5)) - 1, 0), min(int(np.floor(v.max() - 0.5)) + 1, H - 1)
            if c0 > c1 or r0 > r1:
                continue
            dx, dy = np.meshgrid(uu[c0:c1 + 1], vv[r0:r1 + 1])
            e, dist = [], []
            for i in range(3):
                C = np.cross(T[i], T[(i + 1) % 3])
                ei = dx * C[0] + dy * C[1] + C[2]
                e.append(ei)
                g = np.hypot(C[0] / fx, C[1] / fy)
                dist.append(np.abs(ei) / g if g > 0 else np.full_like(ei, np.inf))
            e = np.stack(e)
            inside = (e >= 0).all(0) | (e <= 0).all(0)
            den = e.sum(0)
            with np.errstate(divide="ignore", invalid="ignore"):
                z = np.where(den != 0, (T[0] @ n) / den, -1.0)
            hit = inside & (den != 0) & (z >= znear) & (z <= far)
            near_edge = np.min(dist, axis=0) < edge_tol
            near_clip = (np.abs(z - znear) <= 1e-9 * znear + 1e-12) | (np.abs(z - far) <= 1e-9 * far)
            sl = (k, slice(r0, r1 + 1), slice(c0, c1 + 1))
            amb[sl] |= near_edge | (inside & near_clip)
            depth[sl] = np.where(hit, np.minimum(depth[sl], z), depth[sl])
    depth[np.isinf(depth)] = 0.0
    return depth, amb


def point_masks(points, depth, c2w_list, H, W, fx, fy, cx, cy, r):
    """Mesher.point_masks as the contract states it, in torch CPU with grid_sample.  Returns (seen, forecast, margin):
    margin [n] = per vertex the smallest, over frames, of |z - (d + 0.05)| (where d > 0), the distances of u and v to
    every frustum bound, and |z|."""
    pts = torch.as_tensor(np.asarray(points), dtype=torch.float32)
    depth = torch.as_tensor(np.asarray(depth), dtype=torch.float32)
    c2w_list = torch.as_tensor(np.asarray(c2w_list)).float().reshape(-1, 4, 4)
    n = pts.shape[0]
    seen = torch.zeros(n, dtype=torch.bool)
    fc = torch.zeros(n, dtype=torch.bool)
    margin = torch.full((n,), float("inf"), dtype=torch.float64)
    Kmat = torch.tensor([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]], dtype=torch.float32)
    homo = torch.cat([pts, torch.ones(n, 1)], 1).reshape(-1, 4, 1)
    for i in range(c2w_list.shape[0]):
        w2c = torch.inverse(c2w_list[i])
        cam = (w2c @ homo)[:, :3, :]
        uv = Kmat @ cam
        z = uv[:, -1:] + 1e-8
        uv = uv[:, :2] / z
        u, v, z = uv[:, 0, 0], uv[:, 1, 0], z[:, 0, 0]
        inf = (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1) & (z > 0)
        ff = (u >= -r) & (u <= W - 1 + r) & (v >= -r) & (v <= H - 1 + r) & (z > 0)
        g = uv.reshape(1, 1, -1, 2).clone()
        g[..., 0] = g[..., 0] / (W - 1) * 2.0 - 1.0
        g[..., 1] = g[..., 1] / (H - 1) * 2.0 - 1.0
        d = F.grid_sample(depth[i].reshape(1, 1, H, W), g, padding_mode="border", align_corners=True).reshape(-1)
        front = torch.where(d > 0, z < d + 0.05, torch.ones_like(z, dtype=torch.bool))
        seen |= inf & front
        fc |= (inf & front) | (ff & front)
        m = torch.stack([(u - b).abs() for b in (0.0, W - 1.0, -r, W - 1.0 + r)]
                        + [(v - b).abs() for b in (0.0, H - 1.0, -r, H - 1.0 + r)] + [z.abs()], 1).min(1).values.double()
        # the depth test decides only inside either frustum
        zm = torch.where((d > 0) & (inf | ff), (z - (d + 0.05)).abs(), torch.full_like(z, float("inf"))).double()
        margin = torch.minimum(margin, torch.minimum(m, zm))
    return seen.numpy(), fc.numpy(), margin.numpy()


def face_components(faces, vertices=None):
    """Edge-adjacency components by scipy.sparse.csgraph: labels [F] = smallest face index per component; with vertices,
    also {label: area} (float64 face areas summed with math.fsum) and the total."""
    import math
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    nf = len(faces)
    e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    fid = np.tile(np.arange(nf), 3)
    ok = e[:, 0] != e[:, 1]
    e, fid = np.sort(e[ok], axis=1), fid[ok]
    _, inv = np.unique(e, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    first = np.full(inv.max() + 1 if len(inv) else 0, nf, np.int64)
    np.minimum.at(first, inv, fid)
    g = coo_matrix((np.ones(len(fid)), (fid, first[inv])), shape=(nf, nf))
    _, comp = connected_components(g, directed=False)
    lab_min = np.full(comp.max() + 1 if nf else 0, nf, np.int64)
    np.minimum.at(lab_min, comp, np.arange(nf))
    labels = lab_min[comp]
    if vertices is None:
        return labels
    v = np.asarray(vertices, np.float64)[faces]
    area = 0.5 * np.linalg.norm(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]), axis=1)
    areas = {int(l): math.fsum(area[labels == l]) for l in np.unique(labels)}
    return labels, areas, math.fsum(area)


def obb(points, extend=0.0):
    """Open3D's create_from_points on all points: (center, R, extent) from the population covariance of the convex hull's
    vertices (columns of R by decreasing eigenvalue)."""
    from scipy.spatial import ConvexHull
    p = np.asarray(points, np.float64)
    hv = p[ConvexHull(p).vertices]
    hv = hv[np.lexsort(hv.T[::-1])]          # a canonical order, so that equal vertex sets give equal sums
    mean = hv.mean(0)
    d = hv - mean
    w, V = np.linalg.eigh(d.T @ d / len(hv))
    R = np.ascontiguousarray(V[:, ::-1])
    q = d @ R
    lo, hi = q.min(0), q.max(0)
    return R @ ((lo + hi) / 2) + mean, R, hi - lo + extend


def obb_in_bound(points, center, R, extent):
    d = np.asarray(points, np.float64) - center
    local = d[:, 0:1] * R[0] + d[:, 1:2] * R[1] + d[:, 2:3] * R[2]
    return (np.abs(local) <= extent / 2).all(1), (np.abs(np.abs(local) - extent / 2)).min(1)


def _cut(verts, faces, vmask):
    """faces whose three vertices pass, then unreferenced vertices dropped (order kept)."""
    faces = faces[vmask[faces].all(1)]
    used = np.zeros(len(verts), bool)
    used[faces.reshape(-1)] = True
    remap = np.cumsum(used) - 1
    return verts[used], remap[faces].reshape(-1, 3)


def connected(verts, faces, thr, largest):
    if len(faces) == 0:
        return verts[:0], faces
    labels, areas, total = face_components(faces, verts)
    if largest:
        best = max(areas.items(), key=lambda kv: (kv[1], -kv[0]))[0]
        fm = labels == best
    else:
        fm = np.array([areas[int(l)] > thr * total for l in labels])
    faces = faces[fm]
    used = np.zeros(len(verts), bool)
    used[faces.reshape(-1)] = True
    remap = np.cumsum(used) - 1
    return verts[used], remap[faces].reshape(-1, 3)


def cull_mesh(verts, faces, c2w_list, bound, H, W, fx, fy, cx, cy, radius, thr, largest):
    """Mesher.cull_mesh composed from the restatements: (cull verts, faces), (forecast verts, faces).  `bound` is an
    ndarray AABB [3,2] or None."""
    verts, faces = np.asarray(verts, np.float64), np.asarray(faces, np.int64)
    if bound is not None:
        m = np.all(verts >= bound[:, 0] - 0.001, 1) & np.all(verts <= bound[:, 1] + 0.001, 1)
        verts, faces = _cut(verts, faces, m)
    depth, _ = mesh_depth(verts, faces, c2w_list, H, W, fx, fy, cx, cy)
    seen, fc, _ = point_masks(verts, depth.astype(np.float32), c2w_list, H, W, fx, fy, cx, cy, radius)
    hv, hf = _cut(verts, faces, seen)
    cv, cf = connected(hv, hf, thr, largest)
    if abs(radius) > 0:
        fv, ff = _cut(verts, faces, fc)
        c, R, e = obb(cv)
        inside, _ = obb_in_bound(fv, c, R, e)
        fv, ff = _cut(fv, ff, inside)
        fv, ff = connected(fv, ff, thr, largest)
    else:
        fv, ff = cv, cf
    return (cv, cf), (fv, ff)
