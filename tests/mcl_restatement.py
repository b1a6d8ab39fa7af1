"""Serial restatement of the particle-filter contract of include/goslam_hip.h (gs_mcl_move, gs_mcl_weigh, gs_mcl_estimate,
gs_mcl_resample) and of one tick of the filter built from them: plain loops over the particles in Python integers (the
beams of one particle are a numpy row, so that the shapes of the GPU tests stay runnable).  It shares no code with
csrc/mcl.hip and imports nothing from the package; the tables (headings, beam end points, weights) are made by the one
host function each that both sides call, and handed in by the callers.  tests/test_mcl_cpu.py holds it against
independent models."""
import math

import numpy as np

FREE, UNKNOWN = 254, 205
NO_SCORE = 0xffffffff
NO_BEST = 0xffffffffffffffff
MAX_END = 4000000
MASK64 = (1 << 64) - 1
STATS = 16


def move(particles, rot, noise, odometry, shape):
    """int32 [N,3] of gs_mcl_move: particles and noise [N,3], rot [H,2], odometry (df, dl, dh), shape (n_u, n_v)."""
    particles, rot, noise = np.asarray(particles), np.asarray(rot), np.asarray(noise)
    H = rot.shape[0]
    df, dl, dh = (int(v) for v in odometry)
    out = np.zeros(particles.shape, dtype=np.int32)
    for p in range(particles.shape[0]):
        x, y, h = (int(v) for v in particles[p])
        n0, n1, n2 = (int(v) for v in noise[p])
        c, s = (int(v) for v in rot[h % H])
        f, l = df + n0, dl + n1
        xn = x + ((f * c - l * s + 8192) >> 14)                  # Python's >> floors, as the arithmetic shift does
        yn = y + ((f * s + l * c + 8192) >> 14)
        out[p] = (min(max(xn, 0), 1000 * shape[0] - 1), min(max(yn, 0), 1000 * shape[1] - 1), (h + dh + n2) % H)
    return out


def stands(cells, particle, n_headings, allow_unknown):
    x, y, h = (int(v) for v in particle)
    n_u, n_v = cells.shape
    if not (0 <= x < 1000 * n_u and 0 <= y < 1000 * n_v and 0 <= h < n_headings):
        return False
    c = int(cells[x // 1000, y // 1000])
    return c == FREE or (bool(allow_unknown) and c == UNKNOWN)


def weigh(cost, cells, particles, ends, cap, allow_unknown):
    """(S uint32 [N], best: the python int of gs_mcl_weigh's u64 word): ends [H,B,2]."""
    cost, cells, particles = np.asarray(cost), np.asarray(cells), np.asarray(particles)
    ends = np.asarray(ends).astype(np.int64)
    n_u, n_v = cost.shape
    H = ends.shape[0]
    S = np.full(particles.shape[0], NO_SCORE, dtype=np.int64)
    best = NO_BEST
    for p in range(particles.shape[0]):
        if not stands(cells, particles[p], H, allow_unknown):
            continue
        x, y, h = (int(v) for v in particles[p])
        e = ends[h]
        near = (np.abs(e[:, 0]) <= MAX_END) & (np.abs(e[:, 1]) <= MAX_END)
        cu, cv = (x + e[:, 0]) // 1000, (y + e[:, 1]) // 1000   # numpy's // on integers floors
        inside = near & (cu >= 0) & (cu < n_u) & (cv >= 0) & (cv < n_v)
        total = int(cost[cu[inside], cv[inside]].astype(np.int64).sum()) + int(cap) * int((~inside).sum())
        S[p] = total
        best = min(best, (total << 32) | p)
    return S.astype(np.uint32), best


def estimate(S, particles, rot, lut):
    """(w uint32 [N], cum uint64 [N], stats: 16 python ints, the u64 words) of gs_mcl_estimate."""
    S, particles, rot, lut = np.asarray(S), np.asarray(particles), np.asarray(rot), np.asarray(lut)
    N, L = S.shape[0], lut.shape[0]
    standing = [p for p in range(N) if int(S[p]) != NO_SCORE]
    best = min(((int(S[p]) << 32) | p for p in standing), default=NO_BEST)
    s_min = best >> 32
    w = np.zeros(N, dtype=np.uint32)
    cum = np.zeros(N, dtype=np.uint64)
    sums = [0] * STATS
    sums[2], sums[4] = len(standing), best
    run = 0
    for p in range(N):
        s = int(S[p])
        wt = int(lut[s - s_min]) if s != NO_SCORE and s - s_min < L else 0
        w[p] = wt
        run += wt
        cum[p] = run
        if wt == 0:
            continue
        x, y, h = (int(v) for v in particles[p])
        c, sn = (int(v) for v in rot[h])
        sums[0] += wt
        sums[1] += wt * wt
        sums[3] += 1
        sums[5] += wt * x
        sums[6] += wt * y
        sums[7] += wt * c
        sums[8] += wt * sn
        for at, v in ((9, x * x), (11, y * y), (13, x * y)):
            sums[at] += wt * (v >> 20)
            sums[at + 1] += wt * (v & 0xfffff)
    return w, cum, [v & MASK64 for v in sums]


def resample(cum, particles, W, q):
    """int32 [N,3] of gs_mcl_resample: new particle j copies the smallest i with cum[i] * N > j * W + q."""
    particles = np.asarray(particles)
    cum = [int(v) for v in np.asarray(cum)]
    N = len(cum)
    out = np.zeros((N, 3), dtype=np.int32)
    i = 0                                                       # the thresholds grow with j, so the answer never goes back
    for j in range(N):
        while i < N - 1 and not cum[i] * N > j * W + q:
            i += 1
        out[j] = particles[i]
    return out


def signed(word):
    return word - (1 << 64) if word >> 63 else word


def moments(stats):
    """The exact sums behind the words of `stats`: {"W", "W2", "standing", "positive", "best", "x", "y", "c", "s", "xx",
    "yy", "xy"} in Python integers."""
    return {"W": stats[0], "W2": stats[1], "standing": stats[2], "positive": stats[3], "best": stats[4], "x": stats[5],
            "y": stats[6], "c": signed(stats[7]), "s": signed(stats[8]), "xx": (stats[9] << 20) + stats[10],
            "yy": (stats[11] << 20) + stats[12], "xy": (stats[13] << 20) + stats[14]}


def tick(particles, odometry, noise, ends, cost, cells, rot, lut, cap, allow_unknown, draw):
    """One tick of the filter: move, weigh, estimate, and systematic resampling when 2 W^2 < N sum w^2 (the effective sample
    size W^2 / sum w^2 below N / 2) with q = (draw() * W) >> 32, draw() a 32-bit integer, asked for only then.
    -> (particles after the tick, {"stats", "S", "best", "resampled"}); `ends` None or without a beam: nothing is weighed,
    nothing stands."""
    particles = move(particles, rot, noise, odometry, np.asarray(cells).shape)
    N = particles.shape[0]
    if ends is None or np.asarray(ends).shape[1] == 0:
        return particles, {"stats": [0, 0, 0, 0, NO_BEST] + [0] * 11, "S": np.full(N, NO_SCORE, np.uint32), "best": NO_BEST,
                           "resampled": False}
    S, best = weigh(cost, cells, particles, ends, cap, allow_unknown)
    _, cum, stats = estimate(S, particles, rot, lut)
    W, W2 = stats[0], stats[1]
    resampled = W > 0 and 2 * W * W < N * W2
    if resampled:
        particles = resample(cum, particles, W, (int(draw()) * W) >> 32)
    return particles, {"stats": stats, "S": S, "best": best, "resampled": resampled}


def pose(stats, n_headings):
    """(x, y in milli-cells, heading in steps in [0, H)) of the weighted mean; None when W == 0."""
    m = moments(stats)
    if m["W"] == 0:
        return None
    turn = math.atan2(m["s"], m["c"]) / (2.0 * math.pi) * n_headings
    return m["x"] / m["W"], m["y"] / m["W"], turn % n_headings
