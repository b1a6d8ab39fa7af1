"""Serial restatement of the view-gain contract of include/goslam_hip.h (gs_view_gain): the walk of one ray cell by cell
and the distinct counts of a view with Python sets.  It shares no code with csrc/view_gain.hip or go_slam_amd/view.py;
tests/test_view_gain_cpu.py checks the walk itself against exact rational geometry."""
import numpy as np

MAX_DIR = 32767                        # GS_VIEW_MAX_DIR
MAX_BOX_CELLS = 1 << 20                # GS_VIEW_MAX_BOX_CELLS
INF = 0x3fffffff                       # GS_GEO_INF


def walk(origin, d, dims, range2=None, box=None, state=None, max_unknown=0):
    """The cells one ray visits, in order, as tuples.  `range2` None: no range; `box` None: no box; `state` None: nothing
    stops the ray but the lattice, the box and the range."""
    flat = None if state is None else (state if isinstance(state, bytes) else np.ascontiguousarray(state).tobytes())
    o = tuple(int(v) for v in origin)
    d = tuple(int(v) for v in d)
    n0, n1, n2 = dims
    if not (0 <= o[0] < n0 and 0 <= o[1] < n1 and 0 <= o[2] < n2) or d == (0, 0, 0) or max(abs(v) for v in d) > MAX_DIR:
        return []
    s = [(v > 0) - (v < 0) for v in d]
    w = [abs(v) for v in d]
    axes = [a for a in range(3) if w[a] != 0]
    k = [0, 0, 0]
    cells = []
    unknown = 0
    c = o
    while True:
        cells.append(c)
        if flat is not None:
            st = flat[(c[0] * n1 + c[1]) * n2 + c[2]]
            if st > 1:
                break
            if st == 0:
                unknown += 1
                if unknown == max_unknown:                  # max_unknown 0: no limit
                    break
        best = axes[0]
        for a in axes[1:]:                                  # a beats the best so far only by a strictly earlier crossing
            if (2 * k[a] + 1) * w[best] < (2 * k[best] + 1) * w[a]:
                best = a
        off = [s[0] * k[0], s[1] * k[1], s[2] * k[2]]
        off[best] += s[best]
        nxt = (o[0] + off[0], o[1] + off[1], o[2] + off[2])
        if not (0 <= nxt[0] < n0 and 0 <= nxt[1] < n1 and 0 <= nxt[2] < n2):
            break
        if box is not None and not (box[0] <= off[0] <= box[3] and box[1] <= off[1] <= box[4]
                                    and box[2] <= off[2] <= box[5]):
            break
        if range2 is not None and off[0] * off[0] + off[1] * off[1] + off[2] * off[2] > range2:
            break
        k[best] += 1
        c = nxt
    return cells


def gain(state, origin, dirs, range2, max_unknown=0, box=None):
    """(unknown, free, solid, total): the distinct cells of each kind that the rays `dirs` visit from `origin`."""
    seen = set()
    flat = np.ascontiguousarray(state).tobytes()
    for d in {tuple(int(v) for v in d) for d in dirs}:                                    # a duplicate ray visits what its twin visits
        seen.update(walk(origin, d, state.shape, range2, box, flat, max_unknown))
    kinds = [int(state[c]) for c in seen]
    u, f = kinds.count(0), kinds.count(1)
    return u, f, len(kinds) - u - f, len(kinds)


def gains(state, origins, dirs, range2, max_unknown=0, box=None):
    """uint32 [V,4]: `gain` for every origin."""
    dirs = [tuple(int(v) for v in d) for d in np.asarray(dirs).reshape(-1, 3)]
    return np.array([gain(state, o, dirs, range2, max_unknown, box) for o in np.asarray(origins).reshape(-1, 3)],
                    dtype=np.uint32).reshape(-1, 4)


def full_box(range_cells):
    return (-range_cells,) * 3 + (range_cells,) * 3


def candidates(cost, up_axis, k0, k1, stride, max_candidates):
    """(cells int32 [V,3], cost int32 [V]): the cells with cost < INF on the layers k0 .. k1 of `up_axis` whose two other
    coordinates are multiples of `stride`, by ascending (cost, linear index), the first `max_candidates` of them."""
    rows = []
    for lin, c in enumerate(np.ndindex(*cost.shape)):
        if cost[c] >= INF or not k0 <= c[up_axis] <= k1:
            continue
        if any(c[a] % stride for a in range(3) if a != up_axis):
            continue
        rows.append((int(cost[c]), lin, c))
    rows.sort()
    rows = rows[:max_candidates]
    return (np.array([r[2] for r in rows], dtype=np.int32).reshape(-1, 3),
            np.array([r[0] for r in rows], dtype=np.int32).reshape(-1))
