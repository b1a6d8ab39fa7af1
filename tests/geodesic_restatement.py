"""Serial restatement of the cost-to-go contract of include/goslam_hip.h (gs_geodesic_*): a heap Dijkstra with the
no-corner-cutting move rule and the cap, and the path walk with its tie rule.  It knows nothing of bricks, sweeps or
dirty flags; tests/test_geodesic_cpu.py checks it against scipy's Dijkstra on the explicitly built graph."""
import heapq

import numpy as np

INF = 0x3fffffff
MAX_COST = INF - 1732
MOVES = [(d0, d1, d2) for d0 in (-1, 0, 1) for d1 in (-1, 0, 1) for d2 in (-1, 0, 1) if (d0, d1, d2) != (0, 0, 0)]
WEIGHTS = [{1: 1000, 2: 1414, 3: 1732}[sum(c != 0 for c in d)] for d in MOVES]


def allowed(passable, c, d):
    """Whether the move from cell c by d is allowed: every cell of the box the two ends span is inside and passable."""
    shape = passable.shape
    for a in {0, d[0]}:
        for b in {0, d[1]}:
            for e in {0, d[2]}:
                p = (c[0] + a, c[1] + b, c[2] + e)
                if not all(0 <= p[i] < shape[i] for i in range(3)) or not passable[p]:
                    return False
    return True


def move_masks(passable):
    """bool [26,n0,n1,n2]: `allowed` for every cell and move at once (shifted views of the zero-padded lattice)."""
    passable = np.asarray(passable) != 0
    n0, n1, n2 = passable.shape
    pad = np.zeros((n0 + 2, n1 + 2, n2 + 2), dtype=bool)
    pad[1:-1, 1:-1, 1:-1] = passable
    out = np.ones((26, n0, n1, n2), dtype=bool)
    for m, d in enumerate(MOVES):
        for a in {0, d[0]}:
            for b in {0, d[1]}:
                for e in {0, d[2]}:
                    out[m] &= pad[1 + a:1 + a + n0, 1 + b:1 + b + n1, 1 + e:1 + e + n2]
    return out


def field(passable, seeds, max_cost=MAX_COST):
    """int32 cost [n0,n1,n2] of the contract: 0 at passable in-range seeds, the shortest allowed path's length where it
    is at most max_cost, INF elsewhere."""
    passable = np.asarray(passable) != 0
    assert passable.ndim == 3 and 0 <= max_cost <= MAX_COST
    cost = np.full(passable.shape, INF, dtype=np.int64)
    heap = []
    for s in np.asarray(seeds, dtype=np.int64).reshape(-1, 3):
        s = tuple(int(v) for v in s)
        if all(0 <= s[i] < passable.shape[i] for i in range(3)) and passable[s] and cost[s] != 0:
            cost[s] = 0
            heap.append((0, s))
    heapq.heapify(heap)
    ok = move_masks(passable)
    while heap:
        c_cost, c = heapq.heappop(heap)
        if c_cost > cost[c]:
            continue
        for m, (d, w) in enumerate(zip(MOVES, WEIGHTS)):
            cand = c_cost + w
            if cand > max_cost:
                continue                                    # never stored
            n = (c[0] + d[0], c[1] + d[1], c[2] + d[2])
            if not ok[(m,) + c]:
                continue
            if cand < cost[n]:
                cost[n] = cand
                heapq.heappush(heap, (cand, n))
    return cost.astype(np.int32)


def path(cost, passable, start, max_len):
    """(cells int32 [L,3], n) of gs_geodesic_path: n = 0 for a start outside or at INF, -1 (and no cells) when max_len
    cells do not suffice or no allowed neighbour is finite, else the number of cells of the walk from start to a cell
    of cost 0."""
    passable = np.asarray(passable) != 0
    empty = np.zeros((0, 3), dtype=np.int32)
    cur = tuple(int(v) for v in start)
    if not all(0 <= cur[i] < cost.shape[i] for i in range(3)) or cost[cur] >= INF:
        return empty, 0
    cells = []
    while len(cells) < max_len:
        cells.append(cur)
        if cost[cur] == 0:
            return np.array(cells, dtype=np.int32).reshape(-1, 3), len(cells)
        best = None
        for m, (d, w) in enumerate(zip(MOVES, WEIGHTS)):
            if not allowed(passable, cur, d):
                continue
            n = (cur[0] + d[0], cur[1] + d[1], cur[2] + d[2])
            if cost[n] >= INF:
                continue
            key = (int(cost[n]) + w, m)
            if best is None or key < best[0]:
                best = (key, n)
        if best is None:
            return empty, -1
        cur = best[1]
    return empty, -1


def move_graph(passable):
    """The allowed-move graph as (rows, cols, weights) over linear cell indices, built cell by cell from `allowed`
    (for scipy.sparse.csgraph.dijkstra)."""
    passable = np.asarray(passable) != 0
    n0, n1, n2 = passable.shape
    rows, cols, vals = [], [], []
    for c in np.ndindex(n0, n1, n2):
        if not passable[c]:
            continue
        for d, w in zip(MOVES, WEIGHTS):
            if allowed(passable, c, d):
                rows.append((c[0] * n1 + c[1]) * n2 + c[2])
                cols.append(((c[0] + d[0]) * n1 + c[1] + d[1]) * n2 + c[2] + d[2])
                vals.append(w)
    return rows, cols, vals
