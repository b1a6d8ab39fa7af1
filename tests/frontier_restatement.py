"""Serial restatement of the frontier contract of include/goslam_hip.h (gs_frontier_*): the marking rule cell by cell, the
26-connected components by a flood fill from every unvisited frontier cell in ascending linear order (so the cell a fill
starts from is its component's smallest index), and the table by one loop over the frontier cells.  It knows nothing of
bricks, sweeps, dirty flags or atomics; tests/test_frontier_cpu.py checks it against scipy.ndimage."""
import numpy as np

INF = 0x3fffffff
FACES = [(-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)]
NEIGHBOURS = [(d0, d1, d2) for d0 in (-1, 0, 1) for d1 in (-1, 0, 1) for d2 in (-1, 0, 1) if (d0, d1, d2) != (0, 0, 0)]


def unknown_faces(state, c):
    """The number of face neighbours of cell c that lie inside the lattice and are unknown."""
    n = 0
    for d in FACES:
        p = (c[0] + d[0], c[1] + d[1], c[2] + d[2])
        if all(0 <= p[i] < state.shape[i] for i in range(3)) and state[p] == 0:
            n += 1
    return n


def mark(state, open=None):
    """(frontier uint8 [n0,n1,n2], counts uint32 [4] = unknown, free, solid, frontier cells)."""
    state = np.asarray(state)
    assert state.ndim == 3 and state.dtype == np.uint8
    frontier = np.zeros(state.shape, dtype=np.uint8)
    for c in np.ndindex(*state.shape):
        if state[c] == 1 and (open is None or open[c] != 0) and unknown_faces(state, c) > 0:
            frontier[c] = 1
    counts = np.array([(state == 0).sum(), (state == 1).sum(), (state > 1).sum(), frontier.sum()], dtype=np.uint32)
    return frontier, counts


def labels(frontier):
    """int32 [n0,n1,n2]: -1 off the frontier, else the smallest linear index of the cell's 26-connected component."""
    shape = frontier.shape
    label = np.full(shape, -1, dtype=np.int32)
    for c in np.ndindex(*shape):                            # ascending linear order
        if frontier[c] == 0 or label[c] >= 0:
            continue
        root = int(np.ravel_multi_index(c, shape))
        label[c] = root
        stack = [c]
        while stack:
            a = stack.pop()
            for d in NEIGHBOURS:
                p = (a[0] + d[0], a[1] + d[1], a[2] + d[2])
                if all(0 <= p[i] < shape[i] for i in range(3)) and frontier[p] != 0 and label[p] < 0:
                    label[p] = root
                    stack.append(p)
    return label


def table(state, label, cost=None):
    """The cluster table of the contract, rows by ascending root: {"root", "size", "faces" int32 [K], "sum" int64 [K,3],
    "bbox" int32 [K,6] (mins, then maxes), "best_cost", "best_cell" int32 [K]}."""
    roots = sorted(set(int(v) for v in label.ravel() if v >= 0))
    row = {r: i for i, r in enumerate(roots)}
    K = len(roots)
    size, faces = np.zeros(K, dtype=np.int32), np.zeros(K, dtype=np.int32)
    total = np.zeros((K, 3), dtype=np.int64)
    bbox = np.zeros((K, 6), dtype=np.int32)
    best = [None] * K
    for c in np.ndindex(*label.shape):
        if label[c] < 0:
            continue
        i = row[int(label[c])]
        if size[i] == 0:
            bbox[i] = c + c
        size[i] += 1
        faces[i] += unknown_faces(state, c)
        for a in range(3):
            total[i, a] += c[a]
            bbox[i, a] = min(bbox[i, a], c[a])
            bbox[i, 3 + a] = max(bbox[i, 3 + a], c[a])
        key = (INF if cost is None else int(cost[c]), int(np.ravel_multi_index(c, label.shape)))
        if best[i] is None or key < best[i]:
            best[i] = key
    return {"root": np.array(roots, dtype=np.int32).reshape(K), "size": size, "faces": faces, "sum": total, "bbox": bbox,
            "best_cost": np.array([b[0] for b in best], dtype=np.int32).reshape(K),
            "best_cell": np.array([b[1] for b in best], dtype=np.int32).reshape(K)}


def clusters(state, open=None, cost=None):
    """Everything at once: {"frontier", "label", "counts"} and the table's columns."""
    state = np.asarray(state)
    frontier, counts = mark(state, open)
    label = labels(frontier)
    return {"frontier": frontier, "label": label, "counts": counts, **table(state, label, cost)}
