"""Serial restatement of the line-of-sight contract of include/goslam_hip.h (gs_segment_* / gs_path_*): the supercover
walk, `sees`, the smallest field value along a leg, the sight matrix in the library's bit layout, the leg length and the
shortest shortcut over a path's own cells.  Plain loops over Python integers; it knows nothing of lanes, ballots or LDS.
tests/test_sight_cpu.py checks the walk against an exact rational slab test and the programme against a Dijkstra over the
full visibility graph."""
import math

import numpy as np

MAX_CELLS = 16384                                           # GS_PATH_MAX_CELLS
INF = 0x7fffffff


def sign(v):
    return (v > 0) - (v < 0)


SUBSETS = {s: [t for t in range(1, 8) if t & s == t] for s in range(1, 8)}      # the non-empty subsets of a set of axes


def walk_cells(a, b):
    """Yields the cells of the supercover of the cells a and b in the order of the contract's walk, a first."""
    a = (int(a[0]), int(a[1]), int(a[2]))
    d = (int(b[0]) - a[0], int(b[1]) - a[1], int(b[2]) - a[2])
    w = (abs(d[0]), abs(d[1]), abs(d[2]))
    g = (sign(d[0]), sign(d[1]), sign(d[2]))
    k = [0, 0, 0]
    f = list(a)
    yield a
    while k[0] < w[0] or k[1] < w[1] or k[2] < w[2]:
        live = [i for i in (0, 1, 2) if k[i] < w[i]]
        # axis i crosses at (2 k_i + 1) / (2 w_i): i is among the first when no live axis crosses strictly before it
        first = 0
        for i in live:
            if all((2 * k[i] + 1) * w[j] <= (2 * k[j] + 1) * w[i] for j in live):
                first |= 1 << i
        for t in SUBSETS[first]:
            yield (f[0] + (g[0] if t & 1 else 0), f[1] + (g[1] if t & 2 else 0), f[2] + (g[2] if t & 4 else 0))
        for i in live:
            if first >> i & 1:
                f[i] += g[i]
                k[i] += 1


def walk(a, b):
    """`walk_cells` as a list."""
    return list(walk_cells(a, b))


def inside(c, shape):
    return all(0 <= int(c[i]) < shape[i] for i in range(3))


def sees(passable, a, b):
    """Whether cell a sees cell b over `passable`: both inside and every cell of the supercover passable."""
    if not (inside(a, passable.shape) and inside(b, passable.shape)):
        return False
    return all(passable[c] for c in walk_cells(a, b))       # stops at the first blocked cell


def segment_min(field, a, b):
    """(value, cell) of gs_segment_min: the smallest field value over the supercover and the lowest linear index that
    holds it; (INT32_MIN, -1) for an end outside."""
    if not (inside(a, field.shape) and inside(b, field.shape)):
        return -2 ** 31, -1
    n1, n2 = field.shape[1], field.shape[2]
    return min((int(field[c]), (c[0] * n1 + c[1]) * n2 + c[2]) for c in walk(a, b))


def leg_length(a, b):
    """floor(sqrt(1000000 * |b - a|^2)): milli-voxels."""
    return math.isqrt(1000000 * sum((int(b[i]) - int(a[i])) ** 2 for i in range(3)))


def check_window(L, window):
    if not (1 <= L <= MAX_CELLS and 1 <= window <= max(L - 1, 1)):
        raise ValueError(f"L = {L}, window = {window}")


def sight_matrix(passable, cells, window):
    """uint64 [L, ceil(window / 64)] of gs_path_sight: bit b of row j says that cell j - 1 - b sees cell j."""
    cells = [tuple(int(v) for v in c) for c in np.asarray(cells).reshape(-1, 3)]
    L = len(cells)
    check_window(L, window)
    words = (window + 63) // 64
    rows = [[0] * words for _ in range(L)]
    for j in range(L):
        for b in range(min(window, j)):
            if sees(passable, cells[j - 1 - b], cells[j]):
                rows[j][b // 64] |= 1 << (b % 64)
    return np.array(rows, dtype=np.uint64).reshape(L, words)


def shortcut(sight, cells, window):
    """(index int32 [K], length) of gs_path_shortcut, or (None, None) when the last cell is not reached."""
    cells = np.asarray(cells).reshape(-1, 3)
    L = len(cells)
    check_window(L, window)
    dp, pred = [0] + [INF] * (L - 1), [0] * L
    for j in range(1, L):
        best = None
        for b in range(min(window, j)):
            i = j - 1 - b
            if not (int(sight[j, b // 64]) >> (b % 64) & 1) or dp[i] == INF:
                continue
            cand = dp[i] + leg_length(cells[i], cells[j])
            if cand < INF and (best is None or (cand, i) < best):
                best = (cand, i)
        if best is not None:
            dp[j], pred[j] = best
    if dp[L - 1] == INF:
        return None, None
    index = [L - 1]
    while index[-1] > 0:
        index.append(pred[index[-1]])
    return np.array(index[::-1], dtype=np.int32), dp[L - 1]


def straighten(passable, cells, window):
    """`shortcut` of `sight_matrix`, the window cut to the path as plan.straighten cuts it."""
    L = len(np.asarray(cells).reshape(-1, 3))
    w = max(min(int(window), L - 1), 1)
    return shortcut(sight_matrix(passable, cells, w), cells, w)


def greedy(passable, cells):
    """The rule the programme is not: from each kept cell jump to the farthest later cell it sees.  (index, length)."""
    cells = np.asarray(cells).reshape(-1, 3)
    index, length = [0], 0
    while index[-1] < len(cells) - 1:
        i = index[-1]
        j = max(j for j in range(i + 1, len(cells)) if sees(passable, cells[i], cells[j]))
        length += leg_length(cells[i], cells[j])
        index.append(j)
    return np.array(index, dtype=np.int32), length
