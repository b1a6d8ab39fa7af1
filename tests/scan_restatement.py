"""Serial restatement of the scan contract of include/goslam_hip.h (gs_scan_cast, gs_scan_field, gs_scan_match): the walk
of one beam cell by cell, the likelihood field as two band-limited passes and the correlative score as plain loops over
the yaws and the beams (the translations of a window are numpy slices, so that the shapes of the GPU tests stay
runnable).  It shares no code with csrc/scan.hip; the beam end points come from go_slam_amd.scan.beam_offsets, the one
host function both sides call.  tests/test_scan_cpu.py holds it against independent models."""
import math

import numpy as np

MAX_DIR = 32767                        # GS_VIEW_MAX_DIR
FREE, UNKNOWN = 254, 205
NO_SCORE = 0xffffffff
NO_BEST = 0xffffffffffffffff


def walk(origin, d, shape, range2=None):
    """The cells (u, v) one beam visits on a map of `shape` when nothing stops it but the map and the range, in order."""
    o = (int(origin[0]), int(origin[1]))
    d = (int(d[0]), int(d[1]))
    if not (0 <= o[0] < shape[0] and 0 <= o[1] < shape[1]) or d == (0, 0) or max(abs(d[0]), abs(d[1])) > MAX_DIR:
        return []
    s = [(v > 0) - (v < 0) for v in d]
    w = [abs(v) for v in d]
    k = [0, 0]
    cells = [o]
    while True:
        # axis 1 only by a strictly earlier crossing; an axis the beam does not move along never steps
        a = 1 if w[1] != 0 and (w[0] == 0 or (2 * k[1] + 1) * w[0] < (2 * k[0] + 1) * w[1]) else 0
        off = [s[0] * k[0], s[1] * k[1]]
        off[a] += s[a]
        nxt = (o[0] + off[0], o[1] + off[1])
        if not (0 <= nxt[0] < shape[0] and 0 <= nxt[1] < shape[1]):
            break
        if range2 is not None and off[0] * off[0] + off[1] * off[1] > range2:
            break
        k[a] += 1
        cells.append(nxt)
    return cells


def cast(cells, poses, dirs, range2, stop_unknown):
    """(kind uint8 [P,B], hit int32 [P,B], range_mc int32 [P,B]) of gs_scan_cast."""
    cells = np.asarray(cells)
    poses = np.asarray(poses).reshape(-1, 2)
    dirs = np.asarray(dirs).reshape(poses.shape[0], -1, 2)
    P, B = dirs.shape[:2]
    kind = np.zeros((P, B), dtype=np.uint8)
    hit = np.full((P, B), -1, dtype=np.int32)
    range_mc = np.full((P, B), -1, dtype=np.int32)
    n_v = cells.shape[1]
    for p in range(P):
        for b in range(B):
            for c in walk(poses[p], dirs[p, b], cells.shape, range2):
                value = int(cells[c])
                if value == FREE or (value == UNKNOWN and not stop_unknown):
                    continue
                kind[p, b] = 2 if value == UNKNOWN else 1
                hit[p, b] = c[0] * n_v + c[1]
                du, dv = c[0] - int(poses[p, 0]), c[1] - int(poses[p, 1])
                range_mc[p, b] = math.isqrt(1000000 * (du * du + dv * dv))
                break
    return kind, hit, range_mc


def field(cells, R):
    """uint8 [n_u,n_v] of gs_scan_field: min(d2, R * R + 1) by the two passes of the contract."""
    cells = np.asarray(cells)
    n_u, n_v = cells.shape
    cap = R * R + 1
    first = np.full((n_u, n_v), cap, dtype=np.int64)
    for u in range(n_u):
        for v in range(n_v):
            for k in range(-R, R + 1):
                if 0 <= v + k < n_v and cells[u, v + k] != FREE and cells[u, v + k] != UNKNOWN:
                    first[u, v] = min(first[u, v], k * k)
    out = np.full((n_u, n_v), cap, dtype=np.int64)
    for u in range(n_u):
        for k in range(-R, R + 1):
            if 0 <= u + k < n_u:
                out[u] = np.minimum(out[u], first[u + k] + k * k)
    return out.astype(np.uint8)


def match(cost, cells, offsets, window, cap, allow_unknown):
    """(score uint32 [Y,w_u,w_v], best: the python int of gs_scan_match's u64 word)."""
    cost, cells = np.asarray(cost), np.asarray(cells)
    offsets = np.asarray(offsets)
    n_u, n_v = cost.shape
    u0, v0, w_u, w_v = window
    Y, B = offsets.shape[:2]
    stands = cells[u0:u0 + w_u, v0:v0 + w_v] == FREE
    if allow_unknown:
        stands = stands | (cells[u0:u0 + w_u, v0:v0 + w_v] == UNKNOWN)
    score = np.zeros((Y, w_u, w_v), dtype=np.int64)
    for y in range(Y):
        for b in range(B):
            du, dv = int(offsets[y, b, 0]), int(offsets[y, b, 1])
            add = np.full((w_u, w_v), cap, dtype=np.int64)
            if -32768 <= du <= 32767 and -32768 <= dv <= 32767:
                # the translations (u0 + i, v0 + j) whose end point (u0 + i + du, v0 + j + dv) lies inside the map
                i0, i1 = max(0, -(u0 + du)), min(w_u, n_u - u0 - du)
                j0, j1 = max(0, -(v0 + dv)), min(w_v, n_v - v0 - dv)
                if i0 < i1 and j0 < j1:
                    add[i0:i1, j0:j1] = cost[u0 + du + i0:u0 + du + i1, v0 + dv + j0:v0 + dv + j1]
            score[y] += add
        score[y][~stands] = NO_SCORE
    best = NO_BEST
    flat = score.reshape(-1)
    ok = np.nonzero(flat != NO_SCORE)[0]
    if ok.size:
        index = int(ok[np.argmin(flat[ok])])                            # argmin: the first of the smallest
        best = (int(flat[index]) << 32) | index
    return score.astype(np.uint32), best
