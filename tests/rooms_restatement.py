"""Serial restatement of the room contract of include/goslam_hip.h (gs_room_*), definitions 1 to 7: the core components
by a flood fill in ascending linear order, the cost from geodesic_restatement's Dijkstra, the room labels assigned in
ascending cost order (a cell's parents all cost less, so they are final when the cell's turn comes), the doorways by a
flood fill of the boundary cells and both tables by plain loops.  It knows nothing of bricks, sweeps, dirty flags or
atomics; tests/test_rooms_cpu.py checks it against scipy.ndimage and an independent brute force."""
import numpy as np

import geodesic_restatement as GR

INF = GR.INF
MOVES, WEIGHTS = GR.MOVES, GR.WEIGHTS


def components(mask):
    """int32 [n0,n1,n2]: -1 off the mask, else the smallest linear index of the cell's 26-connected component."""
    shape = mask.shape
    label = np.full(shape, -1, dtype=np.int32)
    for c in np.ndindex(*shape):                            # ascending linear order
        if not mask[c] or label[c] >= 0:
            continue
        root = int(np.ravel_multi_index(c, shape))
        label[c] = root
        stack = [c]
        while stack:
            a = stack.pop()
            for d in MOVES:
                p = (a[0] + d[0], a[1] + d[1], a[2] + d[2])
                if all(0 <= p[i] < shape[i] for i in range(3)) and mask[p] and label[p] < 0:
                    label[p] = root
                    stack.append(p)
    return label


def kept_cores(open_, core, min_core_cells=1):
    """(label int32: the root on the cells of the kept core components, -1 elsewhere; roots and sizes of all components,
    ascending)."""
    label = components((open_ != 0) & (core != 0))
    roots, sizes = np.unique(label[label >= 0], return_counts=True)
    for r, n in zip(roots, sizes):
        if n < min_core_cells:
            label[label == r] = -1
    return label, roots.astype(np.int32), sizes.astype(np.int32)


def room_labels(open_, cost, core_label):
    """int32 R of definition 3, from the kept cores' labels and the cost field."""
    ok = GR.move_masks(open_)
    label = core_label.copy()
    todo = np.argwhere((open_ != 0) & (cost > 0) & (cost < INF))
    order = np.argsort(cost[tuple(todo.T)], kind="stable")
    for c in todo[order]:
        c = tuple(int(v) for v in c)
        best = None
        for m, (d, w) in enumerate(zip(MOVES, WEIGHTS)):
            if not ok[(m,) + c]:
                continue
            q = (c[0] + d[0], c[1] + d[1], c[2] + d[2])
            if int(cost[q]) + w == int(cost[c]):
                assert label[q] >= 0                        # a parent costs less: it was labelled before
                best = int(label[q]) if best is None else min(best, int(label[q]))
        assert best is not None                             # the cost's fixed point: a parent exists
        label[c] = best
    return label


def across(open_ok, label, c):
    """The labels across the allowed moves of the labelled cell c that differ from its own."""
    out = []
    for m, d in enumerate(MOVES):
        if not open_ok[(m,) + c]:
            continue
        q = (c[0] + d[0], c[1] + d[1], c[2] + d[2])
        if label[q] >= 0 and label[q] != label[c]:
            out.append(int(label[q]))
    return out


def cells_table(label, roots):
    """size, sum, bbox of the cells of each root, rows in the order of `roots`."""
    K = len(roots)
    row = {int(r): i for i, r in enumerate(roots)}
    size = np.zeros(K, dtype=np.int32)
    total = np.zeros((K, 3), dtype=np.int64)
    bbox = np.zeros((K, 6), dtype=np.int32)
    for c in np.ndindex(*label.shape):
        if label[c] < 0:
            continue
        i = row[int(label[c])]
        if size[i] == 0:
            bbox[i] = c + c
        size[i] += 1
        for a in range(3):
            total[i, a] += c[a]
            bbox[i, a] = min(bbox[i, a], c[a])
            bbox[i, 3 + a] = max(bbox[i, 3 + a], c[a])
    return size, total, bbox


def segments(open_, core, d2=None, min_core_cells=1, max_cost=GR.MAX_COST):
    """Everything at once: {"label", "cost", "door_label", "counts" (open, core, boundary cells), "rooms": {root, size,
    core_size, sum, bbox, reach}, "doors": {root, size, sum, bbox, room_lo, room_hi, widest_cell, widest_d2}}."""
    open_ = (np.asarray(open_) != 0)
    core = (np.asarray(core) != 0)
    assert open_.ndim == 3 and core.shape == open_.shape
    core_label, all_roots, all_sizes = kept_cores(open_, core, min_core_cells)
    cost = GR.field(open_, np.argwhere(core_label >= 0), max_cost)
    label = room_labels(open_, cost, core_label)
    ok = GR.move_masks(open_)
    boundary = np.zeros(open_.shape, dtype=bool)
    for c in np.ndindex(*open_.shape):
        boundary[c] = label[c] >= 0 and len(across(ok, label, c)) > 0
    door_label = components(boundary)

    roots = np.array(sorted(int(r) for r, n in zip(all_roots, all_sizes) if n >= min_core_cells), dtype=np.int32)
    size, total, bbox = cells_table(label, roots)
    core_size = np.array([(core_label == r).sum() for r in roots], dtype=np.int32).reshape(len(roots))
    reach = np.array([cost[label == r].max() for r in roots], dtype=np.int32).reshape(len(roots))
    rooms = {"root": roots, "size": size, "core_size": core_size, "sum": total, "bbox": bbox, "reach": reach}

    droots = np.array(sorted(set(int(v) for v in door_label.ravel() if v >= 0)), dtype=np.int32)
    D = len(droots)
    dsize, dtotal, dbbox = cells_table(door_label, droots)
    lo, hi = np.zeros(D, dtype=np.int32), np.zeros(D, dtype=np.int32)
    wcell, wd2 = np.zeros(D, dtype=np.int32), np.zeros(D, dtype=np.int32)
    for i, r in enumerate(droots):
        found, best = [], None
        for c in np.argwhere(door_label == r):              # ascending linear order
            c = tuple(int(v) for v in c)
            found += [int(label[c])] + across(ok, label, c)
            w = 0 if d2 is None else max(int(d2[c]), 0)
            if best is None or w > best[0]:                 # ties stay with the lowest index
                best = (w, int(np.ravel_multi_index(c, open_.shape)))
        lo[i], hi[i], wd2[i], wcell[i] = min(found), max(found), best[0], best[1]
    doors = {"root": droots, "size": dsize, "sum": dtotal, "bbox": dbbox, "room_lo": lo, "room_hi": hi,
             "widest_cell": wcell, "widest_d2": wd2}
    counts = np.array([open_.sum(), (open_ & core).sum(), boundary.sum()], dtype=np.int64)
    return {"label": label, "cost": cost, "door_label": door_label, "counts": counts, "rooms": rooms, "doors": doors,
            "core_roots": all_roots, "core_sizes": all_sizes}
