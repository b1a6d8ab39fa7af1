"""NumPy fp64 restatement of the trajectory-evaluation contracts (include/goslam_hip.h gs_traj_world, gs_ape_moments,
gs_ape_stats; kernels in go_slam_amd/csrc/traj_eval.hip), with the same pass structure, reduction order and median
rule, and a running forward-error bound beside every number.

The bound.  u = 2^-53.  A sum of terms a_k that is evaluated in ANY order with a chain of at most L rounded operations
from a term's inputs to the result differs from the exact sum by at most L u sum|a_k| to first order (Higham, Accuracy
and Stability of Numerical Algorithms, 4.2 with gamma_L ~ L u); an error d_k already in a term adds sum|d_k|.  Each
function below counts L for its own longest chain and carries sum|a_k| and sum|d_k| along.  Both the kernel and this
restatement obey the bound against the exact value, so the two differ by at most TWICE the bound: that is the tolerance
of tests/test_traj_eval_gpu.py, no constant is chosen.
"""
import math

import numpy as np

U = 2.0 ** -53
BLOCK = 256                 # TE_BLOCK: frames per block, one per thread
TREE = 8                    # log2(BLOCK): additions on the tree path of one block


# ---------------------------------------------------------------------------------------------- the reduction -----
def _tree(vals, op=np.add):
    """LDS tree of one block: [BLOCK, ...] -> [...], stride 128, 64, ... 1."""
    red = np.array(vals, dtype=np.float64, copy=True)
    w = BLOCK // 2
    while w > 0:
        red[:w] = op(red[:w], red[w:2 * w])
        w //= 2
    return red[0]


def reduce_fixed(terms, op=np.add, identity=0.0):
    """terms [n, ...] (one row per frame, the identity for frames outside the mask) -> the kernels' result: per block
    a tree over its 256 frames; then thread t combines blocks t, t + 256, ... in ascending order and a last tree."""
    terms = np.asarray(terms, dtype=np.float64)
    n = terms.shape[0]
    nblk = (n + BLOCK - 1) // BLOCK
    pad = np.full((nblk * BLOCK,) + terms.shape[1:], identity, dtype=np.float64)
    pad[:n] = terms
    parts = np.stack([_tree(pad[b * BLOCK:(b + 1) * BLOCK], op) for b in range(nblk)]) if nblk else \
        np.zeros((0,) + terms.shape[1:])
    acc = np.full((BLOCK,) + terms.shape[1:], identity, dtype=np.float64)
    for b in range(nblk):
        acc[b % BLOCK] = op(acc[b % BLOCK], parts[b])
    return _tree(acc, op)


def chain_length(n):
    """additions between a term and the final result: the block tree, the serial adds over blocks, the last tree"""
    nblk = max(1, (n + BLOCK - 1) // BLOCK)
    return TREE + (nblk + BLOCK - 1) // BLOCK + TREE


# ---------------------------------------------------------------------------------------------- gs_traj_world -----
def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _qrot(q, p):
    uv = _cross(q[..., :3], p)
    uv = uv + uv
    return (p + q[..., 3:4] * uv) + _cross(q[..., :3], uv)


def _qrot_abs(q, p):
    """the same expression over absolute values: bounds every intermediate magnitude"""
    q, p = np.abs(q), np.abs(p)

    def cross_abs(a, b):
        return np.stack([a[..., 1] * b[..., 2] + a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] + a[..., 0] * b[..., 2],
                         a[..., 0] * b[..., 1] + a[..., 1] * b[..., 0]], axis=-1)
    uv = 2 * cross_abs(q[..., :3], p)
    return p + q[..., 3:4] * uv + cross_abs(q[..., :3], uv)


QROT_OPS = 9                # mul, sub, double, mul, sub, mul, add, add: longest chain through te_qrot, rounded up


def traj_world(w2c, comp):
    """w2c f32 [n,7], comp f32 [7] -> (tq f64 [n,7], mat f64 [n,4,4], bound_tq [n,7], bound_mat [n,4,4])."""
    w = np.asarray(w2c, dtype=np.float32).astype(np.float64)
    c = np.asarray(comp, dtype=np.float32).astype(np.float64).reshape(7)
    n = w.shape[0]
    t, q = w[:, :3], w[:, 3:]
    qi = np.concatenate([-q[:, :3], q[:, 3:]], axis=1)
    ti = -_qrot(qi, t)
    ti_abs = _qrot_abs(qi, t)
    a = np.broadcast_to(c[3:], (n, 4))
    rt = _qrot(a, ti)
    rt_abs = _qrot_abs(a, ti_abs)
    to = c[:3] + rt
    b = qi
    qo = np.stack([((a[:, 3] * b[:, 0] + a[:, 0] * b[:, 3]) + a[:, 1] * b[:, 2]) - a[:, 2] * b[:, 1],
                   ((a[:, 3] * b[:, 1] + a[:, 1] * b[:, 3]) + a[:, 2] * b[:, 0]) - a[:, 0] * b[:, 2],
                   ((a[:, 3] * b[:, 2] + a[:, 2] * b[:, 3]) + a[:, 0] * b[:, 1]) - a[:, 1] * b[:, 0],
                   ((a[:, 3] * b[:, 3] - a[:, 0] * b[:, 0]) - a[:, 1] * b[:, 1]) - a[:, 2] * b[:, 2]], axis=1)
    tq = np.concatenate([to, qo], axis=1)
    qa, qb = np.abs(a), np.abs(b)
    qo_abs = np.stack([qa[:, 3] * qb[:, 0] + qa[:, 0] * qb[:, 3] + qa[:, 1] * qb[:, 2] + qa[:, 2] * qb[:, 1],
                       qa[:, 3] * qb[:, 1] + qa[:, 1] * qb[:, 3] + qa[:, 2] * qb[:, 0] + qa[:, 0] * qb[:, 2],
                       qa[:, 3] * qb[:, 2] + qa[:, 2] * qb[:, 3] + qa[:, 0] * qb[:, 1] + qa[:, 1] * qb[:, 0],
                       qa[:, 3] * qb[:, 3] + qa[:, 0] * qb[:, 0] + qa[:, 1] * qb[:, 1] + qa[:, 2] * qb[:, 2]], axis=1)
    # translation: two rotations and one addition in a row; quaternion: one product, 4 operations deep
    b_t = (2 * QROT_OPS + 1) * U * (np.abs(c[:3]) + rt_abs)
    b_q = 4 * U * qo_abs
    bound_tq = np.concatenate([b_t, b_q], axis=1)
    mat = np.zeros((n, 4, 4))
    bound_mat = np.zeros((n, 4, 4))
    eye = np.eye(3)
    for col in range(3):
        e = np.broadcast_to(eye[col], (n, 3))
        mat[:, :3, col] = _qrot(qo, e)
        # the rotation of a basis vector is quadratic in q: (QROT_OPS + 2 * 4) operations from a's and b's entries
        bound_mat[:, :3, col] = (QROT_OPS + 8) * U * _qrot_abs(qo_abs, e)
    mat[:, :3, 3] = to
    bound_mat[:, :3, 3] = b_t
    mat[:, 3, 3] = 1.0
    return tq, mat, bound_tq, bound_mat


# ---------------------------------------------------------------------------------------------- gs_ape_moments ----
def ape_moments(est, ref, mask=None):
    """-> (moments f64 [17], bound f64 [17]) in the kernel's layout; rows outside the mask are never read."""
    est, ref = np.asarray(est, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    n = est.shape[0]
    valid = np.ones(n, dtype=bool) if mask is None else np.asarray(mask).astype(bool)
    e = np.where(valid[:, None], est, 0.0)
    r = np.where(valid[:, None], ref, 0.0)
    L = chain_length(n)
    cnt = float(reduce_fixed(valid.astype(np.float64)))
    out, bound = np.zeros(17), np.zeros(17)
    out[0] = cnt
    if cnt == 0:
        return out, bound
    s = reduce_fixed(np.concatenate([e, r], axis=1))
    s_abs = np.abs(np.concatenate([e, r], axis=1)).sum(axis=0)
    means = s / cnt
    b_means = (L + 1) * U * s_abs / cnt                              # the sum's chain and the division
    out[1:7], bound[1:7] = means, b_means
    ec = np.where(valid[:, None], e - means[:3], 0.0)
    rc = np.where(valid[:, None], r - means[3:], 0.0)
    # a centred value carries the mean's error and its own subtraction's rounding
    d_ec = np.where(valid[:, None], b_means[:3] + U * np.abs(ec), 0.0)
    d_rc = np.where(valid[:, None], b_means[3:] + U * np.abs(rc), 0.0)
    prod = rc[:, :, None] * ec[:, None, :]                          # [n, ref axis, est axis]
    d_prod = np.abs(rc)[:, :, None] * d_ec[:, None, :] + d_rc[:, :, None] * np.abs(ec)[:, None, :]
    sq = (ec[:, 0] * ec[:, 0] + ec[:, 1] * ec[:, 1]) + ec[:, 2] * ec[:, 2]
    d_sq = (2 * np.abs(ec) * d_ec).sum(axis=1)
    terms = np.concatenate([prod.reshape(n, 9), sq[:, None]], axis=1)
    d_terms = np.concatenate([d_prod.reshape(n, 9), d_sq[:, None]], axis=1)
    S = reduce_fixed(terms)
    # chain: the product (1) or the three-term square (3), the reduction, the division
    Lc = np.array([L + 2] * 9 + [L + 4])
    out[7:17] = S / cnt
    bound[7:17] = (d_terms.sum(axis=0) + Lc * U * np.abs(terms).sum(axis=0)) / cnt
    return out, bound


def umeyama_from_moments(m, with_scale=True):
    """eval_ate.umeyama_alignment from its SVD on (the host part of go_slam_amd.traj_eval.ape)."""
    mx, my, cov, sx = m[1:4], m[4:7], m[7:16].reshape(3, 3), m[16]
    if m[0] < 1:
        raise ValueError("degenerate covariance rank, Umeyama alignment is not possible")
    Um, D, Vt = np.linalg.svd(cov)
    if np.count_nonzero(D > np.finfo(D.dtype).eps) < 2:
        raise ValueError("degenerate covariance rank, Umeyama alignment is not possible")
    S = np.eye(3)
    if np.linalg.det(Um) * np.linalg.det(Vt) < 0.0:
        S[2, 2] = -1.0
    R = Um @ S @ Vt
    c = float(np.trace(np.diag(D) @ S) / sx) if with_scale else 1.0
    return R, my - c * (R @ mx), c


# ---------------------------------------------------------------------------------------------- gs_ape_stats ------
def _sqrt_bound(x, dx):
    """|sqrt(x') - sqrt(x)| for |x' - x| <= dx: always <= sqrt(dx); <= dx / (2 sqrt(x - dx)) when x > dx"""
    b = math.sqrt(dx)
    if x > dx:
        b = min(b, dx / (2.0 * math.sqrt(x - dx)))
    return b


def ape_stats(est, ref, cR, t, mask=None, d_est=None, d_sim=None):
    """-> (err f64 [n] with -1 outside the mask, stats f64 [7] = rmse mean median min max sse std, bound_err [n],
    bound_stats [7]).  d_est: optional per-coordinate error already in `est`; d_sim = (d_cR [3,3], d_t [3]): optional
    error already in the similarity (both zero when kernel and restatement are handed the same inputs)."""
    est, ref = np.asarray(est, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    cR, t = np.asarray(cR, dtype=np.float64).reshape(3, 3), np.asarray(t, dtype=np.float64).reshape(3)
    n = est.shape[0]
    valid = np.ones(n, dtype=bool) if mask is None else np.asarray(mask).astype(bool)
    e = np.where(valid[:, None], est, 0.0)
    r = np.where(valid[:, None], ref, 0.0)
    p = ((cR[None, :, 0] * e[:, 0:1] + cR[None, :, 1] * e[:, 1:2]) + cR[None, :, 2] * e[:, 2:3]) + t
    p_abs = np.abs(e) @ np.abs(cR).T + np.abs(t)
    d = r - p
    d_d = 4 * U * p_abs + U * np.abs(d)                              # mul, add, add, add; the subtraction
    if d_est is not None:
        d_d = d_d + np.asarray(d_est) @ np.abs(cR).T
    if d_sim is not None:
        d_d = d_d + np.abs(e) @ np.asarray(d_sim[0]).T + np.asarray(d_sim[1])
    err = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    d_err = np.sqrt((d_d ** 2).sum(axis=1)) + 4 * U * err           # the norm is 1-Lipschitz; square, 2 adds, sqrt
    err = np.where(valid, err, -1.0)
    d_err = np.where(valid, d_err, 0.0)
    ev = np.where(valid, err, 0.0)
    L = chain_length(n)
    cnt = float(reduce_fixed(valid.astype(np.float64)))
    stats, bound = np.full(7, np.nan), np.full(7, np.nan)
    if cnt == 0:
        stats[5] = 0.0
        return err, stats, d_err, bound
    s1 = float(reduce_fixed(ev))
    s2 = float(reduce_fixed(ev * ev))
    b_s1 = d_err.sum() + L * U * ev.sum()
    b_s2 = (2 * ev * d_err).sum() + (L + 1) * U * (ev * ev).sum()
    mean, b_mean = s1 / cnt, (b_s1 + U * abs(s1)) / cnt
    msq, b_msq = s2 / cnt, (b_s2 + U * s2) / cnt
    stats[0], bound[0] = math.sqrt(msq), _sqrt_bound(msq, b_msq) + U * math.sqrt(msq)
    stats[1], bound[1] = mean, b_mean
    stats[5], bound[5] = s2, b_s2
    stats[3] = float(reduce_fixed(np.where(valid, err, np.inf), np.minimum, np.inf))
    stats[4] = float(reduce_fixed(np.where(valid, err, -np.inf), np.maximum, -np.inf))
    bound[3] = bound[4] = d_err.max()                                # order statistics are 1-Lipschitz in the sup norm
    # median by rank counting: ties broken by index, the two middle ranks averaged
    idx = np.arange(n)
    less = (err[None, :] < err[:, None]) | ((err[None, :] == err[:, None]) & (idx[None, :] < idx[:, None]))
    rank = (less & valid[None, :]).sum(axis=1)
    c = int(cnt)
    lo = err[valid & (rank == (c - 1) // 2)]
    hi = err[valid & (rank == c // 2)]
    assert lo.shape == (1,) and hi.shape == (1,)
    stats[2], bound[2] = 0.5 * (lo[0] + hi[0]), d_err.max() + U * max(lo[0], hi[0])
    cen = np.where(valid, err - mean, 0.0)
    d_cen = np.where(valid, d_err + b_mean + U * np.abs(cen), 0.0)
    s3 = float(reduce_fixed(cen * cen))
    b_s3 = (2 * np.abs(cen) * d_cen + d_cen ** 2).sum() + (L + 1) * U * (cen * cen).sum()
    var, b_var = s3 / cnt, (b_s3 + U * s3) / cnt
    stats[6], bound[6] = math.sqrt(var), _sqrt_bound(var, b_var) + U * math.sqrt(var)
    return err, stats, d_err, bound


# ---------------------------------------------------------------------------------------------- end to end --------
def alignment_bound(moments, b_moments, R, t, c):
    """How far (cR, t) can move when the 17 moments move by b_moments, to first order.

    cov -> (U, D, V): Weyl moves each singular value by at most |dcov|_2; the rotation U S V^T of the orthogonal
    Procrustes problem moves by at most 2 |dcov|_F / g with g = D_2 + s D_3 the smallest sum of two (signed) singular
    values (Soderkvist 1993, Perturbation analysis of the orthogonal Procrustes problem, eq. 3.6's denominator).  LAPACK's
    own backward error in the 3x3 SVD, p(3) u |cov|_2 with p(3) taken as 30, is added to |dcov|: it is the same for
    every caller but this bound is also used against a different evaluation of the same moments.  c = tr(DS) / var
    and t = my - c R mx follow by the product rule."""
    mx, my, cov, var = moments[1:4], moments[4:7], moments[7:16].reshape(3, 3), moments[16]
    Um, D, Vt = np.linalg.svd(cov)
    dcov = float(np.linalg.norm(b_moments[7:16])) + 30 * U * float(D[0])
    sign = -1.0 if np.linalg.det(Um) * np.linalg.det(Vt) < 0.0 else 1.0
    g = D[1] + sign * D[2]
    dR = 2 * dcov / g if g > 0 else np.inf
    dtr = 3 * dcov
    dc = (dtr + abs(c) * b_moments[16]) / var + 2 * U * abs(c)
    dcR = dc + abs(c) * dR + 2 * U * abs(c)                          # per entry of cR, |R_ij| <= 1
    dt = b_moments[4:7] + dcR * np.abs(mx).sum() + abs(c) * (np.abs(R) @ b_moments[1:4]) \
        + 4 * U * (np.abs(my) + abs(c) * (np.abs(R) @ np.abs(mx)))
    return np.full((3, 3), dcR), dt


def ape(est, ref, mask=None):
    """moments -> host SVD -> statistics, as go_slam_amd.traj_eval.ape: a dict of the statistics and of `bound`, the
    end-to-end bound per statistic, which includes how the alignment moves with the moments' rounding."""
    m, bm = ape_moments(est, ref, mask)
    R, t, c = umeyama_from_moments(m)
    d_sim = alignment_bound(m, bm, R, t, c)
    err, stats, d_err, bound = ape_stats(est, ref, c * R, t, mask, d_sim=d_sim)
    names = ("rmse", "mean", "median", "min", "max", "sse", "std")
    out = dict(zip(names, stats.tolist()))
    out.update(count=int(m[0]), rotation=R, translation=t, scale=c, errors=err,
               bound=dict(zip(names, bound.tolist())), moments=m, moments_bound=bm)
    return out
