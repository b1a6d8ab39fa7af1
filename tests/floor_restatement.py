"""Serial restatement of the drivable-floor kernels (csrc/floor.hip; contract: include/goslam_hip.h, gs_floor_*), written
from the contract's rules and not from the kernels: plain numpy, integers only.

`columns` tries the positions of the band from the lowest up, and decides each from the counts of solid and free cells
in its headroom; `footprint` visits the disc's offsets one by one over the padded maps.  tests/test_floor_cpu.py holds
both against independent models (a per-column search over every position; scipy's rank filters).
"""
import numpy as np

MAP_FREE, MAP_OCCUPIED, MAP_UNKNOWN = 254, 0, 205
WHY_NONE, WHY_NO_FLOOR, WHY_NEAR_NO_FLOOR, WHY_STEP = 0, 1, 2, 3


def positions(state, up_axis, up_sign):
    """state [nx,ny,nz] as [n_u,n_v,n_a]: the up axis last, position p increasing along it."""
    s = np.moveaxis(np.asarray(state), up_axis, 2)
    return s[:, :, ::-1] if up_sign < 0 else s


def columns(state, up_axis, up_sign, p0, p1, H):
    """gs_floor_columns -> (floor int16 [n_u,n_v], kind uint8 [n_u,n_v])."""
    s = positions(state, up_axis, up_sign)
    n_u, n_v, n = s.shape
    assert up_sign in (1, -1) and 0 <= p0 <= p1 < n and H >= 1
    solid = np.concatenate([np.zeros((n_u, n_v, 1), np.int64), np.cumsum(s == 2, axis=2)], axis=2)   # cells below p
    free = np.concatenate([np.zeros((n_u, n_v, 1), np.int64), np.cumsum(s == 1, axis=2)], axis=2)
    floor = np.full((n_u, n_v), -1, dtype=np.int16)
    kind = np.full((n_u, n_v), 255, dtype=np.uint8)
    for p in range(max(p0, 1), p1 + 1):
        top = min(p + H, n)                                    # the cells beyond the lattice are unseen, never solid
        stand = (s[:, :, p - 1] == 2) & (solid[:, :, top] - solid[:, :, p] == 0)
        strict = stand & (p + H <= n) & (free[:, :, top] - free[:, :, p] == H)
        new = stand & (kind == 255)                            # the lowest stand wins
        floor[new] = p if up_sign > 0 else n - 1 - p
        kind[new] = np.where(strict[new], 1, 2)
    lo, hi = max(p0 - 1, 0), min(p1 + H - 1, n - 1)
    window = s[:, :, lo:hi + 1]
    never_seen = ~(window == 2).any(axis=2) & (window == 0).any(axis=2)
    none = kind == 255
    kind[none] = np.where(never_seen[none], 0, 3)
    return floor, kind


def disc(R2):
    """The offsets (du, dv) with du^2 + dv^2 <= R2."""
    r = int(np.floor(np.sqrt(R2)))
    while (r + 1) * (r + 1) <= R2:
        r += 1
    while r * r > R2:
        r -= 1
    return [(du, dv) for du in range(-r, r + 1) for dv in range(-r, r + 1) if du * du + dv * dv <= R2], r


def footprint(floor, kind, R2, S):
    """gs_floor_footprint -> (cells uint8, why uint8, rough int16), all [n_u,n_v]."""
    return footprint_rules(kind, footprint_scan(floor, kind, R2), S)


def footprint_scan(floor, kind, R2):
    """What the disc of every column holds, whatever S is: (a column of kind 3, a column of kind 0 or 2 or off the map,
    the largest height difference to a column of kind 1 or 2)."""
    floor, kind = np.asarray(floor).astype(np.int64), np.asarray(kind)
    assert 2 <= R2 <= 1024
    n_u, n_v = kind.shape
    offsets, r = disc(R2)
    kpad = np.zeros((n_u + 2 * r, n_v + 2 * r), dtype=np.uint8)            # outside the map: kind 0
    fpad = np.zeros((n_u + 2 * r, n_v + 2 * r), dtype=np.int64)
    kpad[r:r + n_u, r:r + n_v] = kind
    fpad[r:r + n_u, r:r + n_v] = floor
    near_blocked = np.zeros((n_u, n_v), dtype=bool)
    near_unsure = np.zeros((n_u, n_v), dtype=bool)
    worst = np.zeros((n_u, n_v), dtype=np.int64)
    for du, dv in offsets:
        kq = kpad[r + du:r + du + n_u, r + dv:r + dv + n_v]
        fq = fpad[r + du:r + du + n_u, r + dv:r + dv + n_v]
        near_blocked |= kq == 3
        near_unsure |= (kq == 0) | (kq == 2)
        has_floor = (kq == 1) | (kq == 2)
        worst = np.maximum(worst, np.where(has_floor, np.abs(fq - floor), 0))
    return near_blocked, near_unsure, worst


def footprint_rules(kind, scan, S):
    """The contract's rules over `footprint_scan`'s result."""
    kind = np.asarray(kind)
    near_blocked, near_unsure, worst = scan
    assert S >= 0
    cells = np.full(kind.shape, MAP_FREE, dtype=np.uint8)
    why = np.zeros(kind.shape, dtype=np.uint8)
    # the rules from the last to the first: an earlier rule overwrites a later one
    cells[(kind == 2) | near_unsure] = MAP_UNKNOWN
    step = worst > S
    cells[step], why[step] = MAP_OCCUPIED, WHY_STEP
    cells[near_blocked], why[near_blocked] = MAP_OCCUPIED, WHY_NEAR_NO_FLOOR
    cells[kind == 0], why[kind == 0] = MAP_UNKNOWN, WHY_NONE
    cells[kind == 3], why[kind == 3] = MAP_OCCUPIED, WHY_NO_FLOOR
    rough = np.where((kind == 1) | (kind == 2), worst, 0).astype(np.int16)
    return cells, why, rough
