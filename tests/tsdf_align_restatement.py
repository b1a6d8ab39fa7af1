"""Restatement of csrc/tsdf_align.hip (include/goslam_hip.h: gs_tsdf_align_system, gs_tsdf_align_step) in NumPy, with
one rounding per operation: np.float32 arrays for the per-pixel arithmetic, np.float64 for the sums, Python floats (IEEE
doubles) for the 6 x 6 solve and the retraction.  The summation order is written out literally: a thread's samples in
increasing order, the wave's butterfly v += v[lane ^ m], the four waves as ((w0 + w1) + w2) + w3, the chunks in
increasing order.  It imports nothing from the package; `chunk` is an argument (tests read gs_tsdf_align_chunk)."""
import math

import numpy as np

F = np.float32
THREADS, WAVE = 256, 64
ROW = 32                                    # H 21, b 6, cost 27, count 28, sq 29, considered 30, 0
DEFAULT_LEVELS = ((4, 10), (2, 10), (1, 5))


def lerp(p, q, s):
    return p + s * (q - p)


def pixel_terms(tsdf, weight, depth_map, pose, stride, intr, lo, voxel, max_depth=math.inf, min_weight=1.0, huber=0.5):
    """What gs_tsdf_align_system computes per sampled pixel of one pose, in sample order s = (iv / stride) * ceil(w /
    stride) + iu / stride: {"considered", "valid": bool [S], "f", "wt": float32 [S], "J": float32 [S,6], "q", "pw":
    float32 [S,3]}.  Rows that are not valid hold whatever the clamped gather gave."""
    tsdf, weight = np.ascontiguousarray(tsdf, F), np.ascontiguousarray(weight, F)
    nx, ny, nz = tsdf.shape
    h, w = depth_map.shape
    fx, fy, cx, cy = (F(v) for v in intr)
    lo, voxel = [F(v) for v in lo], F(voxel)
    max_depth, min_weight, huber = F(max_depth), F(min_weight), F(huber)
    m = np.asarray(pose, np.float64).reshape(3, 4).astype(F)                  # (float) of each fp64 entry
    iv, iu = np.meshgrid(np.arange(0, h, stride), np.arange(0, w, stride), indexing="ij")
    iv, iu = iv.reshape(-1), iu.reshape(-1)
    d = np.ascontiguousarray(depth_map, F)[iv, iu]
    with np.errstate(all="ignore"):
        considered = d > 0
        valid = considered & (d <= max_depth)
        px = (iu.astype(F) - cx) / fx * d
        py = (iv.astype(F) - cy) / fy * d
        q = [(m[r, 0] * px + m[r, 1] * py) + m[r, 2] * d for r in range(3)]
        pw = [q[r] + m[r, 3] for r in range(3)]
        g = [(pw[r] - lo[r]) / voxel for r in range(3)]
        a = [np.floor(x) for x in g]
        for x, n in zip(a, (nx, ny, nz)):
            valid &= (x >= 0) & (x < F(n - 1))                                 # a NaN fails
        ai = [np.where(valid, x, F(0)).astype(np.int64) for x in a]
        at = (ai[0] * ny + ai[1]) * nz + ai[2]
        offs = [(i * ny + j) * nz + k for i in (0, 1) for j in (0, 1) for k in (0, 1)]      # v000 v001 v010 .. v111
        wc = [weight.reshape(-1)[at + o] for o in offs]
        for c in wc:
            valid &= c >= min_weight
        v000, v001, v010, v011, v100, v101, v110, v111 = (tsdf.reshape(-1)[at + o] for o in offs)
        sx, sy, sz = (g[r] - a[r] for r in range(3))
        z00, z01, z10, z11 = lerp(v000, v001, sz), lerp(v010, v011, sz), lerp(v100, v101, sz), lerp(v110, v111, sz)
        x0, x1 = lerp(z00, z01, sy), lerp(z10, z11, sy)
        f = lerp(x0, x1, sx)
        valid &= np.abs(f) < F(1)
        y00, y01, y10, y11 = lerp(v000, v010, sy), lerp(v001, v011, sy), lerp(v100, v110, sy), lerp(v101, v111, sy)
        n = [x1 - x0, lerp(z01, z11, sx) - lerp(z00, z10, sx), lerp(y01, y11, sx) - lerp(y00, y10, sx)]
        gw = [c / voxel for c in n]
        J = np.stack([gw[0], gw[1], gw[2], q[1] * gw[2] - q[2] * gw[1], q[2] * gw[0] - q[0] * gw[2],
                      q[0] * gw[1] - q[1] * gw[0]], axis=1)
        af = np.abs(f)
        wt = np.where(af <= huber, F(1), huber / af)
    assert J.dtype == F and f.dtype == F and wt.dtype == F
    return {"considered": considered, "valid": valid, "f": f, "wt": wt, "J": J, "q": np.stack(q, 1), "pw": np.stack(pw, 1)}


def sample_rows(t):
    """float64 [S,32]: what each sampled pixel adds to out's row (zeros where it is skipped)."""
    S = t["f"].shape[0]
    rows = np.zeros((S, ROW), np.float64)
    with np.errstate(all="ignore"):
        fd, wd, Jd = t["f"].astype(np.float64), t["wt"].astype(np.float64), t["J"].astype(np.float64)
        wj = wd[:, None] * Jd
        at = 0
        for i in range(6):
            for j in range(i, 6):
                rows[:, at] = wj[:, i] * Jd[:, j]
                at += 1
            rows[:, 21 + i] = wj[:, i] * fd
        rows[:, 27] = (wd * fd) * fd
        rows[:, 28] = 1.0
        rows[:, 29] = fd * fd
    rows[~t["valid"]] = 0.0
    rows[:, 30] = t["considered"]
    return rows


def chunked_sum(rows, chunk):
    """The contract's order.  Adding the +0.0 of a skipped sample changes no bit: a running sum that starts at +0.0
    is never -0.0."""
    S = rows.shape[0]
    n_chunks = -(-S // chunk)
    padded = np.zeros((n_chunks * chunk, ROW), np.float64)
    padded[:S] = rows
    rounds = padded.reshape(n_chunks, chunk // THREADS, THREADS, ROW)
    acc = np.zeros((n_chunks, THREADS, ROW), np.float64)
    for r in range(chunk // THREADS):                      # thread t: samples t, t + 256, ...
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


def system(tsdf, weight, depth, frame, pose, stride, intr, lo, voxel, chunk, max_depth=math.inf, min_weight=1.0,
           huber=0.5):
    """gs_tsdf_align_system: float64 [B,32].  depth [k,h,w], frame [B], pose float64 [B,3,4]."""
    pose = np.asarray(pose, np.float64).reshape(-1, 3, 4)
    out = np.zeros((pose.shape[0], ROW), np.float64)
    for b in range(pose.shape[0]):
        fr = int(frame[b])
        if not 0 <= fr < depth.shape[0]:
            continue
        t = pixel_terms(tsdf, weight, depth[fr], pose[b], stride, intr, lo, voxel, max_depth, min_weight, huber)
        out[b] = chunked_sum(sample_rows(t), chunk)
    return out


def retract(m, x):
    """The step's pose update on a [3][4] list of Python floats: o += x[0:3], P = dR R, R = P (I - (P^T P - I) / 2)."""
    hx, hy, hz = x[3] * 0.5, x[4] * 0.5, x[5] * 0.5
    ln = math.sqrt(((1.0 + hx * hx) + hy * hy) + hz * hz)
    a, b, c, d = 1.0 / ln, hx / ln, hy / ln, hz / ln
    aa, bb, cc, dd = a * a, b * b, c * c, d * d
    dR = [[((aa + bb) - cc) - dd, 2.0 * (b * c - a * d), 2.0 * (b * d + a * c)],
          [2.0 * (b * c + a * d), ((aa - bb) + cc) - dd, 2.0 * (c * d - a * b)],
          [2.0 * (b * d - a * c), 2.0 * (c * d + a * b), ((aa - bb) - cc) + dd]]
    P = [[(dR[i][0] * m[0][j] + dR[i][1] * m[1][j]) + dR[i][2] * m[2][j] for j in range(3)] for i in range(3)]
    E = [[((P[0][i] * P[0][j] + P[1][i] * P[1][j]) + P[2][i] * P[2][j]) - (1.0 if i == j else 0.0) for j in range(3)]
         for i in range(3)]
    return [[P[i][j] - 0.5 * ((P[i][0] * E[0][j] + P[i][1] * E[1][j]) + P[i][2] * E[2][j]) for j in range(3)]
            + [m[i][3] + x[i]] for i in range(3)]


def solve(row, lam_rel, lam_abs):
    """x = -A^-1 b by the contract's Cholesky, or None when a pivot fails.  row: 32 Python floats."""
    A = [[0.0] * 6 for _ in range(6)]
    at = 0
    for i in range(6):
        for j in range(i, 6):
            A[i][j] = A[j][i] = row[at]
            at += 1
    for i in range(6):
        A[i][i] = (A[i][i] + lam_rel * A[i][i]) + lam_abs
    L = [[0.0] * 6 for _ in range(6)]
    for j in range(6):
        s = A[j][j]
        for k in range(j):
            s = s - L[j][k] * L[j][k]
        if not s > 0.0:
            return None
        L[j][j] = math.sqrt(s)
        for i in range(j + 1, 6):
            t = A[i][j]
            for k in range(j):
                t = t - L[i][k] * L[j][k]
            L[i][j] = t / L[j][j]
    y = [0.0] * 6
    for i in range(6):
        t = row[21 + i]
        for k in range(i):
            t = t - L[i][k] * y[k]
        y[i] = t / L[i][i]
    z = [0.0] * 6
    for i in range(5, -1, -1):
        t = y[i]
        for k in range(5, i, -1):
            t = t - L[k][i] * z[k]
        z[i] = t / L[i][i]
    return [-v for v in z]


def step(out, pose, lam_rel=1e-6, lam_abs=1e-9, min_count=64):
    """gs_tsdf_align_step: (new pose float64 [B,3,4], trace float64 [B,4] = cost, count, considered, status)."""
    pose = np.array(pose, np.float64).reshape(-1, 3, 4)
    trace = np.zeros((pose.shape[0], 4), np.float64)
    for b in range(pose.shape[0]):
        row = [float(v) for v in out[b]]
        x = None if row[28] < float(min_count) else solve(row, float(lam_rel), float(lam_abs))
        trace[b] = (row[27], row[28], row[30], 0.0 if x is None else 1.0)
        if x is not None:
            pose[b] = np.array(retract(pose[b].tolist(), x), np.float64)
    return pose, trace


def align(tsdf, weight, depth, frame, pose, intr, lo, voxel, chunk, levels=DEFAULT_LEVELS, huber=0.5,
          max_depth=math.inf, min_weight=1.0, lam_rel=1e-6, lam_abs=1e-9, min_count=64):
    """TSDFVolume.align's sequence: per level (stride, iterations) system and step, then one closing system at the last
    level's stride.  -> (pose [B,3,4], closing rows [B,32], trace [iterations,B,4])."""
    pose = np.array(pose, np.float64).reshape(-1, 3, 4)
    trace = []
    for stride, iters in levels:
        for _ in range(iters):
            out = system(tsdf, weight, depth, frame, pose, stride, intr, lo, voxel, chunk, max_depth, min_weight, huber)
            pose, tr = step(out, pose, lam_rel, lam_abs, min_count)
            trace.append(tr)
    closing = system(tsdf, weight, depth, frame, pose, levels[-1][0], intr, lo, voxel, chunk, max_depth, min_weight, huber)
    return pose, closing, np.array(trace, np.float64).reshape(len(trace), pose.shape[0], 4)


# ---- the three-plane scene of the tests ---------------------------------------------------------------------------
SCENE_DIMS, SCENE_VOXEL, SCENE_TRUNC = (37, 31, 45), 0.05, 0.2
SCENE_LO = (-0.2, -0.2, 0.0)                # lattice indices 4, 4 and 40 are x = 0, y = 0 and z = 2
SCENE_H, SCENE_W = 48, 64
SCENE_INTR = (0.9 * SCENE_W, 0.9 * SCENE_W, SCENE_W / 2 - 0.5, SCENE_H / 2 - 0.5)
PLANES_ON, PLANES_OFF = (0.0, 0.0, 2.0), (0.013, 0.021, 1.987)


def rotation(omega):
    """exp of a rotation vector, float64 (Rodrigues): how the tests build poses and starts, never the code under test."""
    omega = np.asarray(omega, np.float64)
    th = float(np.linalg.norm(omega))
    K = np.array([[0, -omega[2], omega[1]], [omega[2], 0, -omega[0]], [-omega[1], omega[0], 0]])
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + math.sin(th) / th * K + (1 - math.cos(th)) / th ** 2 * (K @ K)


def scene_pose():
    """The true camera-to-world pose [3,4]: at (0.95, 0.8, 0.35), looking at the corner region so that every pixel sees
    one of the three planes and each plane fills a good share of the image."""
    o = np.array([0.95, 0.8, 0.35])
    fwd = np.array([0.35, 0.3, 1.45]) - o
    fwd /= np.linalg.norm(fwd)
    right = np.cross(np.array([0.0, 1.0, 0.0]), fwd)
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    return np.concatenate([np.stack([right, down, fwd], 1), o[:, None]], 1)


def scene_depth(pose, planes, h=SCENE_H, w=SCENE_W, intr=SCENE_INTR):
    """float32 [h,w]: depth along the optical axis to the nearest of the planes x = px, y = py, z = pz, from inside the
    room x > px, y > py, z < pz (float64, rounded once)."""
    fx, fy, cx, cy = intr
    v, u = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    ray = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1) @ pose[:, :3].T
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (np.asarray(planes)[None, None, :] - pose[:, 3][None, None, :]) / ray
    t = np.where(t > 0, t, np.inf)
    return t.min(-1).astype(F)


def scene_volume(planes, dims=SCENE_DIMS, lo=SCENE_LO, voxel=SCENE_VOXEL, trunc=SCENE_TRUNC):
    """(tsdf, weight) float32 [nx,ny,nz]: min of the three plane distances over trunc, clipped to [-1, 1]; weight 1."""
    ax = [lo[a] + voxel * np.arange(dims[a], dtype=np.float64) for a in range(3)]
    X, Y, Z = np.meshgrid(*ax, indexing="ij")
    sdf = np.minimum(np.minimum(X - planes[0], Y - planes[1]), planes[2] - Z)
    return np.clip(sdf / trunc, -1.0, 1.0).astype(F), np.ones(dims, F)


def displaced(pose, metres, degrees, rng):
    """`pose` moved by `metres` along a random direction and turned by `degrees` about a random axis (about the camera
    centre, the step's own convention)."""
    v, ax = rng.normal(size=3), rng.normal(size=3)
    v, ax = v / np.linalg.norm(v) * metres, ax / np.linalg.norm(ax) * math.radians(degrees)
    return np.concatenate([rotation(ax) @ pose[:, :3], (pose[:, 3] + v)[:, None]], 1)


def pose_error(pose, truth):
    """(metres, degrees) between two [3,4] poses; the angle from |Ra - Rb|_F = 2 sqrt(2) sin(theta / 2)."""
    dm = float(np.linalg.norm(pose[:, 3] - truth[:, 3]))
    s = float(np.linalg.norm(pose[:, :3] - truth[:, :3])) / (2.0 * math.sqrt(2.0))
    return dm, math.degrees(2.0 * math.asin(min(1.0, s)))
