"""NumPy restatement of the mesh-evaluation contracts (include/goslam_neus.h gs_nn_*, gs_icp_moments;
go_slam_amd/neus/mesh_eval.py), serial and without a GPU.

- nn: brute force over every reference point, d2 = dx*dx + dy*dy + dz*dz left to right, the smallest index on equal
  d2, the radius test d2 < r*r;
- icp: Open3D's point-to-point loop, the moments summed in the documented order (sums, then centred products);
- sample_surface: trimesh.sample.sample_surface;
- metrics: eval_mesh's five numbers from two distance arrays.
"""
import numpy as np


def transform_points(p, T):
    p = np.asarray(p, dtype=np.float64).reshape(-1, 3)
    T = np.asarray(T, dtype=np.float64).reshape(4, 4)
    return np.stack([((T[r, 0] * p[:, 0] + T[r, 1] * p[:, 1]) + T[r, 2] * p[:, 2]) + T[r, 3] for r in range(3)], 1)


def nn(q, r, max_distance=None, transform=None, chunk=2048):
    """(d2 float64 [M], index int32 [M]) by brute force."""
    q = np.asarray(q, dtype=np.float64).reshape(-1, 3)
    r = np.asarray(r, dtype=np.float64).reshape(-1, 3)
    if transform is not None:
        q = transform_points(q, transform)
    d2 = np.full(len(q), np.inf)
    idx = np.full(len(q), -1, dtype=np.int32)
    if len(r):
        for s in range(0, len(q), chunk):
            a = q[s:s + chunk]
            dx = a[:, None, 0] - r[None, :, 0]
            dy = a[:, None, 1] - r[None, :, 1]
            dz = a[:, None, 2] - r[None, :, 2]
            D = (dx * dx + dy * dy) + dz * dz
            j = np.argmin(D, axis=1)                 # the first minimum: the smallest index of a tie
            d2[s:s + chunk] = D[np.arange(len(a)), j]
            idx[s:s + chunk] = j
    if max_distance is not None:
        out = ~(d2 < max_distance * max_distance)
        d2[out] = np.inf
        idx[out] = -1
    return d2, idx


def moments(src, tgt, idx, d2, T):
    """count, sum d2, centroids, centred cross-covariance sum (t - t_mean)(s - s_mean)^T."""
    ok = idx >= 0
    s = transform_points(src, T)[ok]
    t = np.asarray(tgt, dtype=np.float64)[idx[ok]]
    cnt = float(ok.sum())
    if cnt == 0:
        return cnt, 0.0, np.zeros(3), np.zeros(3), np.zeros((3, 3))
    ms, mt = s.sum(0) / cnt, t.sum(0) / cnt
    C = (t - mt).T @ (s - ms)
    return cnt, float(d2[ok].sum()), ms, mt, C


def umeyama(cnt, ms, mt, C):
    if cnt == 0:
        return np.eye(4)
    U, _, Vt = np.linalg.svd(C / cnt)
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2, 2] = -1.0
    T = np.eye(4)
    T[:3, :3] = U @ S @ Vt
    T[:3, 3] = mt - T[:3, :3] @ ms
    return T


def icp(src, tgt, threshold, trans_init=None, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6):
    """(T, fitness, inlier_rmse, iterations)."""
    src = np.asarray(src, dtype=np.float64).reshape(-1, 3)
    T = np.eye(4) if trans_init is None else np.array(trans_init, dtype=np.float64)

    def evaluate(T):
        d2, idx = nn(src, tgt, threshold, T)
        m = moments(src, tgt, idx, d2, T)
        fit = m[0] / len(src) if len(src) else 0.0
        rmse = np.sqrt(m[1] / m[0]) if m[0] > 0 else 0.0
        return m, fit, rmse

    m, fit, rmse = evaluate(T)
    it = 0
    for it in range(1, max_iteration + 1):
        T = umeyama(m[0], m[2], m[3], m[4]) @ T
        pf, pr = fit, rmse
        m, fit, rmse = evaluate(T)
        if abs(pf - fit) < relative_fitness and abs(pr - rmse) < relative_rmse:
            break
    return T, fit, rmse, it


def sample_surface(vertices, faces, count, random=np.random):
    tri = np.asarray(vertices, dtype=np.float64)[np.asarray(faces)]
    o = tri[:, 0]
    e = tri[:, 1:] - o[:, None]
    c = np.cross(e[:, 0], e[:, 1])
    w = np.cumsum(np.sqrt((c * c).sum(1)) / 2.0)
    f = np.searchsorted(w, random.random(count) * w[-1])
    u = random.random((count, 2, 1))
    u[u.sum(1).reshape(-1) > 1.0] -= 1.0
    u = np.abs(u)
    return (e[f] * u).sum(1) + o[f]


def metrics(d_acc, d_comp, dist_th):
    acc, comp = np.mean(d_acc) * 100, np.mean(d_comp) * 100
    ar = np.mean((d_acc < dist_th).astype(np.float32)) * 100
    cr = np.mean((d_comp < dist_th).astype(np.float32)) * 100
    with np.errstate(invalid="ignore"):          # both ratios 0: NaN, as in the reference
        f = (2.0 * ar * cr) / (ar + cr)
    return {"accuracy": acc, "completion": comp, "accuracy_ratio": ar, "completion_ratio": cr, "f_score": f}


def eval_mesh(est_v, est_f, gt_v, gt_f, n, dist_th, random=np.random):
    est = sample_surface(est_v, est_f, n, random)
    gt = sample_surface(gt_v, gt_f, n, random)
    d_comp = np.sqrt(nn(gt, est)[0])
    d_acc = np.sqrt(nn(est, gt)[0])
    return metrics(d_acc, d_comp, dist_th)
