"""The particle-filter restatement (tests/mcl_restatement.py) against independent models, and the host side of
go_slam_amd/mcl.py, without a GPU: the move against exact rational rotation, the weigh against a per-particle brute force,
the estimate against Python integers at the contract's extremes, the resampling against numpy.searchsorted, the closed
loop on the recovery scene of DESIGN.md section 36 (the filter tracks within a cell where the reported odometry alone
ends three cells off), the argument errors, the text round trip, the kernels' resources from hipcc, and that none of it
touches a device."""
import math
import os
import re
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import mcl_restatement as R                                    # noqa: E402
import scan_restatement as SR                                  # noqa: E402
import test_scan_cpu as SC                                     # noqa: E402  (the recovery scene)

from go_slam_amd import mcl as M                               # noqa: E402
from go_slam_amd import scan as S                              # noqa: E402

# ---- the closed loop's fixed inputs (the issue's; shared with tests/test_mcl_gpu.py) ------------------------------------
LOOP_H, LOOP_BEAMS, LOOP_RANGE, LOOP_R, LOOP_N = 360, 60, 30, 6, 512
LOOP_START = (10500, 10500, 0)
LOOP_ROUTE = [(1000, 0, 0)] * 18 + [(300, 0, 10)] * 9 + [(1000, 0, 0)] * 15
LOOP_SIGMAS = (100, 50, 1)
LOOP_SEED_SIGMAS = (1000, 1000, 3)
LOOP_SEEDS = (0, 1, 2)
LOOP_DEAD_RECKONED_CELLS = 3.05
# what the restatement's loop gets for seeds 0, 1, 2 (worst position error in cells, worst heading error in steps), as
# DESIGN.md section 38 records them; test_closed_loop_tracks_within_a_cell prints and checks them
LOOP_RECORDED = {0: (0.6597, 2.783), 1: (0.6548, 2.969), 2: (0.6736, 2.377)}
_CACHE = {}


def reported(t, step):
    """The odometry the filter is told at tick t: 5 % long, and a heading step too many every third tick."""
    return (round(1.05 * step[0]), step[1], step[2] + (1 if t % 3 == 0 else 0))


def loop_tables():
    """(cells, cost, rot, lut) of the loop, once."""
    if "tables" not in _CACHE:
        cells = SC.scene()
        _CACHE["tables"] = (cells, SR.field(cells, LOOP_R), M.heading_table(LOOP_H), M.weight_table(LOOP_BEAMS))
        for a in _CACHE["tables"]:
            a.setflags(write=False)
    return _CACHE["tables"]


def loop_truth():
    """[(x, y, h)] after each tick: the route applied without noise by the restatement's move."""
    if "truth" not in _CACHE:
        cells, _, rot, _ = loop_tables()
        p = np.array([LOOP_START], dtype=np.int32)
        out = []
        for step in LOOP_ROUTE:
            p = R.move(p, rot, np.zeros((1, 3), np.int32), step, cells.shape)
            out.append(tuple(int(v) for v in p[0]))
        _CACHE["truth"] = out
    return _CACHE["truth"]


def loop_scans():
    """[(ranges in cells, NaN without a hit; angles)] per tick: cast from the true cell by the scan restatement."""
    if "scans" not in _CACHE:
        cells = SC.scene()
        angles = S.beam_angles(LOOP_BEAMS, 360.0)
        scans = []
        for x, y, h in loop_truth():
            dirs = S.beam_directions(angles, 2.0 * math.pi * h / LOOP_H)
            kind, _, range_mc = SR.cast(cells, [(x // 1000, y // 1000)], dirs[None], LOOP_RANGE ** 2, True)
            scans.append((np.where(kind[0] == 1, range_mc[0] / 1000.0, np.nan), angles))
        _CACHE["scans"] = scans
    return _CACHE["scans"]


def loop_ends(t):
    ranges, angles = loop_scans()[t]
    return M.beam_ends(ranges, angles, LOOP_H, 1.0, 0.0, float(LOOP_RANGE))


def heading_apart(a, b, H=LOOP_H):
    d = abs(a - b) % H
    return min(d, H - d)


def run_restatement_loop(seed, n=LOOP_N, kidnap=None):
    """The restatement's filter through the route: [(position error in cells, heading error in steps, best mean cost,
    standing, resampled)] per tick."""
    cells, cost, rot, lut = loop_tables()
    rng = np.random.default_rng(seed)
    p = np.rint(np.array(LOOP_START) + rng.standard_normal((n, 3)) * np.array(LOOP_SEED_SIGMAS)).astype(np.int64)
    p[:, 0] = np.clip(p[:, 0], 0, 1000 * cells.shape[0] - 1)
    p[:, 1] = np.clip(p[:, 1], 0, 1000 * cells.shape[1] - 1)
    p[:, 2] %= LOOP_H
    p = p.astype(np.int32)
    rows = []
    for t, (step, true) in enumerate(zip(LOOP_ROUTE, loop_truth())):
        noise = np.rint(rng.standard_normal((n, 3)) * np.array(LOOP_SIGMAS)).astype(np.int32)
        ends = loop_ends(t)
        p, info = R.tick(p, reported(t, step), noise, ends, cost, cells, rot, lut, LOOP_R ** 2 + 1, False,
                         lambda: int(rng.integers(0, 1 << 32)))
        est = R.pose(info["stats"], LOOP_H)
        assert est is not None, f"tick {t}: no particle has weight"
        rows.append((math.hypot(est[0] - true[0], est[1] - true[1]) / 1000.0, heading_apart(est[2], true[2]),
                     (info["best"] >> 32) / ends.shape[1], R.moments(info["stats"])["standing"], info["resampled"]))
    return rows


# ---- move ---------------------------------------------------------------------------------------------------------------
def test_move_equals_exact_rotation_within_the_tables_error():
    """x' - x is round((f c - l s) / 2^14) with (c, s) the rounded table: against the exact (f cos - l sin) the table
    costs at most (|f| + |l|) / 2^15 (half a unit of 2^-14 per entry) and the final rounding half a milli-cell; the bound
    asked for is that plus nothing, and at most 1 + (|f| + |l|) / 2^15 milli-cells as the issue states it."""
    H = 360
    rot = M.heading_table(H)
    rng = np.random.default_rng(5)
    n = 400
    parts = np.stack([rng.integers(400000, 600000, n), rng.integers(400000, 600000, n), rng.integers(0, H, n)], 1).astype(np.int32)
    noise = np.stack([rng.integers(-3000, 3000, n), rng.integers(-3000, 3000, n), rng.integers(-400, 400, n)], 1).astype(np.int32)
    odo = (40000, -7000, -3)
    out = R.move(parts, rot, noise, odo, (1024, 1024))
    for p in range(n):
        f, l = odo[0] + int(noise[p, 0]), odo[1] + int(noise[p, 1])
        yaw = 2.0 * math.pi * int(parts[p, 2]) / H
        ex = Fraction(f) * Fraction(math.cos(yaw)) - Fraction(l) * Fraction(math.sin(yaw))
        ey = Fraction(f) * Fraction(math.sin(yaw)) + Fraction(l) * Fraction(math.cos(yaw))
        bound = Fraction(1, 2) + Fraction(abs(f) + abs(l), 1 << 15) + Fraction(1, 1000)     # 1/1000: cos and sin in float64
        assert abs(int(out[p, 0]) - int(parts[p, 0]) - ex) <= bound and bound <= 1 + Fraction(abs(f) + abs(l), 1 << 15)
        assert abs(int(out[p, 1]) - int(parts[p, 1]) - ey) <= bound
        assert int(out[p, 2]) == (int(parts[p, 2]) + odo[2] + int(noise[p, 2])) % H and 0 <= int(out[p, 2]) < H


def test_move_wraps_the_heading_and_clamps_at_the_four_borders():
    rot = M.heading_table(4)
    shape = (3, 5)
    parts = np.array([[100, 100, 2], [2900, 100, 0], [100, 4900, 1], [100, 100, 3], [1500, 2500, 0], [1500, 2500, 1]], np.int32)
    noise = np.array([[0, 0, -7], [0, 0, 9], [0, 0, 0], [0, 0, -1], [0, 0, -4], [-2000, 5, 0]], np.int32)
    out = R.move(parts, rot, noise, (500, 0, 0), shape)
    # heading 2 looks along -u, 0 along +u, 1 along +v, 3 along -v
    assert out.tolist() == [[0, 100, 3], [2999, 100, 1], [100, 4999, 1], [100, 0, 2], [2000, 2500, 0], [1495, 1000, 1]]
    far = R.move(np.array([[1500, 2500, 0]], np.int32), rot, np.array([[1 << 20, -(1 << 20), -(1 << 20)]], np.int32),
                 (1 << 20, -(1 << 20), -(1 << 20)), shape)
    assert far.tolist() == [[2999, 0, (-(1 << 21)) % 4]]
    # a rounding that needs the floor of the shift: f c - l s + 8192 negative
    one = R.move(np.array([[1500, 2500, 0]], np.int32), M.heading_table(360)[:50], np.array([[0, 0, 0]], np.int32), (-3, 0, 0), shape)
    assert one.tolist() == [[1497, 2500, 0]]


# ---- weigh --------------------------------------------------------------------------------------------------------------
def brute_weigh(cost, cells, particles, ends, cap, allow_unknown):
    S = []
    for x, y, h in particles.tolist():
        n_u, n_v = cells.shape
        ok = 0 <= x < 1000 * n_u and 0 <= y < 1000 * n_v and 0 <= h < ends.shape[0]
        if ok:
            c = int(cells[x // 1000, y // 1000])
            ok = c == 254 or (allow_unknown and c == 205)
        if not ok:
            S.append(R.NO_SCORE)
            continue
        total = 0
        for ex, ey in ends[h].tolist():
            tx, ty = x + ex, y + ey
            u, v = math.floor(Fraction(tx, 1000)), math.floor(Fraction(ty, 1000))
            if abs(ex) > 4000000 or abs(ey) > 4000000 or not (0 <= u < n_u and 0 <= v < n_v):
                total += cap
            else:
                total += int(cost[u, v])
        S.append(total)
    standing = [(s << 32) | p for p, s in enumerate(S) if s != R.NO_SCORE]
    return np.array(S, dtype=np.uint32), min(standing, default=R.NO_BEST)


def weigh_inputs(shape, n, H, B, seed):
    """Particles on and off free cells and on the borders, end points that are negative, tiny, across a cell's edge, far
    beyond the limit and exactly at it."""
    rng = np.random.default_rng(seed)
    cells = SC.random_map(shape, seed) if shape != (48, 40) else np.array(SC.scene())
    parts = np.stack([rng.integers(0, 1000 * shape[0], n), rng.integers(0, 1000 * shape[1], n), rng.integers(0, H, n)], 1)
    parts[: min(n, 4)] = [[0, 0, 0], [1000 * shape[0] - 1, 1000 * shape[1] - 1, H - 1], [0, 1000 * shape[1] - 1, 0],
                          [1000 * shape[0] - 1, 0, H // 2]][: min(n, 4)]
    ends = rng.integers(-3000, 3001, (H, B, 2))
    special = [(-1, -1), (-1000, -1001), (-999, 999), (0, 0), (4000000, 0), (4000001, 0), (0, -4000001), (-4000000, -4000000),
               (0x7fffffff, 5), (5, -0x7fffffff), (-500, 500), (-501, 499)]
    for k, e in enumerate(special):
        ends[k % H, (k // H) % B] = e
    return cells, parts.astype(np.int32), ends.astype(np.int32)


@pytest.mark.parametrize("shape,n,H,B", [((48, 40), 120, 7, 13), ((1, 1), 5, 1, 1), ((9, 30), 64, 4, 65)])
@pytest.mark.parametrize("allow_unknown", [False, True])
def test_weigh_equals_a_brute_force(shape, n, H, B, allow_unknown):
    cells, parts, ends = weigh_inputs(shape, n, H, B, 3)
    cost = SR.field(cells, 3)
    want = brute_weigh(cost, cells, parts, ends, 10, allow_unknown)
    got = R.weigh(cost, cells, parts, ends, 10, allow_unknown)
    assert np.array_equal(got[0], want[0]) and got[1] == want[1]
    if shape == (48, 40):
        assert 0 < int((got[0] != R.NO_SCORE).sum()) < n


def test_weigh_on_a_map_without_a_free_cell():
    cells = np.full((6, 7), 205, dtype=np.uint8)
    _, parts, ends = weigh_inputs((6, 7), 20, 3, 5, 1)
    cost = SR.field(cells, 2)
    S_, best = R.weigh(cost, cells, parts, ends, 5, False)
    assert (S_ == R.NO_SCORE).all() and best == R.NO_BEST
    S_, best = R.weigh(cost, cells, parts, ends, 5, True)       # unknown cells carry a robot now; no site: all cap
    assert (S_ == 5 * 5).all() and best == (25 << 32)
    w, cum, stats = R.estimate(np.full(20, R.NO_SCORE, np.uint32), parts, M.heading_table(3), M.weight_table(5))
    assert not w.any() and not cum.any() and stats == [0, 0, 0, 0, R.NO_BEST] + [0] * 11


# ---- estimate -----------------------------------------------------------------------------------------------------------
def test_estimate_sums_at_the_contracts_extremes():
    """N = 65536 particles of weight 2^20 at x = y = 1 023 999: every word stays below 2^57 and nothing wraps."""
    N, x = 65536, 1023999
    parts = np.tile(np.array([[x, x, 0]], np.int32), (N, 1))
    rot = M.heading_table(1)
    w, cum, stats = R.estimate(np.zeros(N, np.uint32), parts, rot, np.array([1 << 20], np.uint32))
    W = N << 20
    assert (w == 1 << 20).all() and int(cum[-1]) == W and int(cum[0]) == 1 << 20
    m = R.moments(stats)
    assert m == {"W": W, "W2": N << 40, "standing": N, "positive": N, "best": 0, "x": W * x, "y": W * x, "c": W << 14, "s": 0,
                 "xx": W * x * x, "yy": W * x * x, "xy": W * x * x}
    assert all(v < 1 << 57 for v in stats) and stats[15] == 0
    assert M.moments(stats) == m
    est = M.pose_from_moments(m, (0.0, 0.0), 1.0, 1)
    assert est["cov"] == ((0.0, 0.0), (0.0, 0.0)) and est["milli"] == (float(x), float(x)) and est["ess"] == N


def test_estimate_against_python_integers():
    rng = np.random.default_rng(11)
    N, H = 1500, 360
    rot, lut = M.heading_table(H), M.weight_table(60)
    parts = np.stack([rng.integers(0, 1024000, N), rng.integers(0, 1024000, N), rng.integers(0, H, N)], 1).astype(np.int32)
    S_ = rng.integers(40, 40 + 2 * len(lut), N).astype(np.uint32)
    S_[rng.random(N) < 0.2] = R.NO_SCORE
    w, cum, stats = R.estimate(S_, parts, rot, lut)
    s_min = min(int(s) for s in S_ if s != R.NO_SCORE)
    ws = [int(lut[int(s) - s_min]) if s != R.NO_SCORE and int(s) - s_min < len(lut) else 0 for s in S_]
    assert w.tolist() == ws and cum.tolist() == np.cumsum(np.array(ws, dtype=object)).tolist()
    m = R.moments(stats)
    assert m["W"] == sum(ws) and m["W2"] == sum(v * v for v in ws) and m["positive"] == sum(v > 0 for v in ws)
    assert m["standing"] == int((S_ != R.NO_SCORE).sum()) and 0 < m["positive"] < m["standing"]
    assert m["best"] == min((int(s) << 32) | p for p, s in enumerate(S_) if s != R.NO_SCORE)
    assert m["c"] == sum(v * int(rot[h, 0]) for v, h in zip(ws, parts[:, 2])) and m["c"] != 0
    assert m["s"] == sum(v * int(rot[h, 1]) for v, h in zip(ws, parts[:, 2]))
    assert m["xy"] == sum(v * int(x) * int(y) for v, x, y in zip(ws, parts[:, 0], parts[:, 1]))
    assert m["xx"] == sum(v * int(x) ** 2 for v, x in zip(ws, parts[:, 0]))
    assert m["x"] == sum(v * int(x) for v, x in zip(ws, parts[:, 0]))


# ---- resample -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 7, 64, 1000])
def test_resample_equals_searchsorted(n):
    rng = np.random.default_rng(n)
    w = rng.integers(0, 1 << 20, n)
    w[rng.random(n) < 0.3] = 0
    w[n // 2] = 1 << 20
    cum = np.cumsum(w).astype(np.uint64)
    W = int(cum[-1])
    parts = np.stack([np.arange(n), rng.integers(0, 99, n), rng.integers(0, 9, n)], 1).astype(np.int32)
    for q in (0, W - 1, W // 3):
        got = R.resample(cum, parts, W, q)
        scaled = np.array([int(c) * n for c in cum], dtype=object)
        want = [int(np.searchsorted(scaled, j * W + q, side="right")) for j in range(n)]
        assert got[:, 0].tolist() == want and np.array_equal(got, parts[want])
        copies = np.bincount(got[:, 0], minlength=n)
        assert all(copies[i] >= 1 for i in range(n) if int(w[i]) * n >= W)        # a share of 1 / N or more survives
        assert all(copies[i] == 0 for i in range(n) if w[i] == 0)


# ---- the host side ------------------------------------------------------------------------------------------------------
def test_tables():
    rot = M.heading_table(360)
    assert rot.dtype == np.int32 and rot[0].tolist() == [16384, 0] and rot[90].tolist() == [0, 16384]
    assert np.abs(np.hypot(rot[:, 0], rot[:, 1]) - 16384).max() < 1.0
    lut = M.weight_table(60)
    assert lut.dtype == np.uint32 and lut[0] == 1 << 20 and lut[-1] >= 1 and len(lut) == 222
    assert [int(v) for v in lut[:3]] == [math.floor((1 << 20) * math.exp(-d / 16.0)) for d in range(3)]
    assert len(M.weight_table(10, 2.0)) == 111 and len(M.weight_table(4096, 15.0)) <= 65536
    assert len(M.weight_table(1, 15.0, squash=1e-9)) == 65536
    angles = S.beam_angles(8, 360.0)
    ranges = np.array([1.0, 2.0, np.nan, 0.5, 40.0, 3.0, np.inf, 1.5])
    ends = M.beam_ends(ranges, angles, 4, 0.5, 0.6, 30.0)
    keep = S.valid_beams(ranges, 0.6, 30.0)
    assert ends.shape == (4, 4, 2) and ends.dtype == np.int32 and keep.sum() == 4
    for k in range(4):
        for b, (r, a) in enumerate(zip(ranges[keep], angles[keep])):
            assert ends[k, b].tolist() == [round(2000 * r * math.cos(a + k * math.pi / 2)), round(2000 * r * math.sin(a + k * math.pi / 2))]
    # beam_offsets at a thousand times the resolution: the same end points up to the rounding rule at exact halves
    off = S.beam_offsets(ranges, angles, 2.0 * math.pi * np.arange(4) / 4, 0.0005, 0.6, 30.0)
    assert np.abs(off - ends).max() <= 1
    assert M.beam_ends([np.nan], [0.0], 3, 1.0).shape == (3, 0, 2)
    assert M.odometry_steps(0.5, -0.25, math.pi / 2, 0.05, 360) == (10000, -5000, 90)
    nz = M.motion_noise(1000, (100, 50, 1), torch.Generator().manual_seed(3))
    assert nz.dtype == torch.int32 and tuple(nz.shape) == (1000, 3) and 80 < float(nz[:, 0].double().std()) < 120
    assert torch.equal(nz, M.motion_noise(1000, (100, 50, 1), torch.Generator().manual_seed(3)))
    assert not M.motion_noise(5, (0, 0, 0)).any()


def test_refusals_come_before_any_device(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(M._lib, "lib", no_device)
    monkeypatch.setattr(torch.Tensor, "cuda", no_device)
    parts = torch.zeros((4, 3), dtype=torch.int32)
    rot, noise = M.heading_table(4), np.zeros((4, 3), np.int32)
    cost = torch.zeros((3, 5), dtype=torch.uint8)
    ends = np.zeros((4, 2, 2), np.int32)
    lut = M.weight_table(10)
    bad = [lambda: M.move(parts.long(), rot, noise, (0, 0, 0), (3, 5)), lambda: M.move(parts[:, :2], rot, noise, (0, 0, 0), (3, 5)),
           lambda: M.move(parts, rot, noise, (0, 0), (3, 5)), lambda: M.move(parts, rot, noise, ((1 << 20) + 1, 0, 0), (3, 5)),
           lambda: M.move(parts, rot, noise, (0, 0, 0.5), (3, 5)), lambda: M.move(parts, rot, noise, (0, 0, 0), (0, 5)),
           lambda: M.move(parts, rot, noise, (0, 0, 0), (3, 1025)), lambda: M.move(parts, rot[:, :1], noise, (0, 0, 0), (3, 5)),
           lambda: M.move(parts, rot, noise[:3], (0, 0, 0), (3, 5)), lambda: M.move(parts, rot, noise, (0, 0, 0), (3, 5)),
           lambda: M.weigh(cost, cost[:2], parts, ends, 5), lambda: M.weigh(cost, cost, parts, ends, 0),
           lambda: M.weigh(cost, cost, parts, ends, 227), lambda: M.weigh(cost, cost, parts, ends, 5, 1),
           lambda: M.weigh(cost, cost, parts, ends[:, :0], 5), lambda: M.weigh(cost, cost, parts, ends[0], 5),
           lambda: M.weigh(cost.float(), cost, parts, ends, 5), lambda: M.weigh(cost, cost, parts, ends, 5),
           lambda: M.estimate(np.zeros(3, np.uint32), parts, rot, lut), lambda: M.estimate(np.zeros(4, np.uint32), parts[:0], rot, lut),
           lambda: M.estimate(np.zeros(4, np.uint32), parts, rot, lut[:0]), lambda: M.estimate(np.zeros(4, np.uint32), parts, rot, lut),
           lambda: M.resample(np.ones(4, np.uint64), parts, 0, 0), lambda: M.resample(np.ones(4, np.uint64), parts, 5, 5),
           lambda: M.resample(np.ones(4, np.uint64), parts, (1 << 36) + 1, 0), lambda: M.resample(np.ones(4, np.uint64), parts, 5, -1),
           lambda: M.resample(np.ones(3, np.uint64), parts, 5, 0), lambda: M.resample(np.ones(4, np.uint64), parts, 5, 0),
           lambda: M.heading_table(0), lambda: M.heading_table(1025), lambda: M.weight_table(0), lambda: M.weight_table(10, 0.0),
           lambda: M.beam_ends([1.0], [0.0, 1.0], 4, 1.0), lambda: M.beam_ends([1.0], [0.0], 4, 0.0),
           lambda: M.odometry_steps(1e9, 0.0, 0.0, 0.05, 360), lambda: M.odometry_steps(math.nan, 0.0, 0.0, 0.05, 360),
           lambda: M.motion_noise(4, (1, 2)), lambda: M.motion_noise(4, (1, 2, -1)), lambda: M.moments([0] * 15)]
    for n, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"call {n} was not refused")
    grid = SC.scene_grid()
    for kw in ({"n_particles": 0}, {"n_particles": 65537}, {"headings": 0}, {"headings": 1025}, {"n_beams": 0}, {"radius_cells": 16},
               {"sigma_cells": 0.0}, {"noise": (1, 2)}, {"noise_rate": (0, 0, -1)}, {"allow_unknown": 1}, {"seed": -1},
               {"lost_ticks": 0}, {"min_range": 5.0, "max_range": 1.0}):
        with pytest.raises(ValueError):
            M.ParticleFilter(grid, **{"n_beams": 60, **kw})
    with pytest.raises(ValueError):
        M.ParticleFilter({"cells": np.zeros((3, 3)), "origin": (0, 0), "resolution": 1.0}, n_beams=60)
    for scanner, drift in (({"beam": 3}, None), ({"beams": 0}, None), ({"beams": 8}, {"scale": 0.0}), ({"beams": 8}, {"turn": 1})):
        with pytest.raises(ValueError):
            M.track_on_map(grid, [], scanner, drift=drift)


def test_config_key_and_text_round_trip():
    assert M.mcl_config(None) is None and M.mcl_config({"enable": False, "up_axis": 7}) is None
    cfg = M.mcl_config({"up_axis": 2, "height": [0.1, 0.3]})
    assert cfg == {"up_axis": 2, "height": (0.1, 0.3), "beams": 360, "fov_deg": 360.0, "max_range": None, "every": 5,
                   "particles": 2048, "headings": 360, "drift": {"scale": 1.0, "yaw_deg_per_m": 0.0}, "seed": 0}
    full = {"enable": True, "up_axis": 1, "height": (0.0, 1.0), "beams": 90, "fov_deg": 270.0, "max_range": 4.0, "every": 2,
            "particles": 512, "headings": 180, "drift": {"scale": 1.05, "yaw_deg_per_m": -2.0}, "seed": 4}
    assert M.mcl_config(full)["drift"] == {"scale": 1.05, "yaw_deg_per_m": -2.0} and M.mcl_config(full)["particles"] == 512
    for key, value in (("up_axis", 3), ("height", (1.0, 0.0)), ("beams", 0), ("fov_deg", 0), ("max_range", -1.0), ("every", 0),
                       ("particles", 0), ("particles", 65537), ("headings", 1025), ("drift", {"scale": 0}), ("drift", {"x": 1}),
                       ("drift", {"yaw_deg_per_m": math.inf}), ("drift", 3), ("seed", -1), ("seed", 1.5), ("enable", 1),
                       ("n_yaw", 8)):
        with pytest.raises(ValueError, match="fuse_from_config: tsdf.esdf.mcl"):
            M.mcl_config({**full, key: value})
    with pytest.raises(ValueError, match="tsdf.esdf.mcl"):
        M.mcl_config({"height": (0, 1)})
    rows = [{"true_x": 0.1, "true_y": -1 / 3, "true_yaw": math.pi, "est_x": 1e-17, "est_y": 2.5, "est_yaw": -0.0, "error_m": 0.1 + 0.2,
             "yaw_error": 5e-324, "ess": 1234.5678, "best_mean_cost": 1 / 7, "n_standing": 2048, "resampled": 1, "lost": 0,
             "relocalized": 0},
            {"true_x": 3.0, "true_y": 4.0, "true_yaw": 0.0, "est_x": math.nan, "est_y": math.nan, "est_yaw": math.nan,
             "error_m": math.inf, "yaw_error": math.inf, "ess": 0.0, "best_mean_cost": math.inf, "n_standing": 0, "resampled": 0,
             "lost": 1, "relocalized": 1}]
    result = {"rows": rows, "particles": 2048, "headings": 360, "ticks": 2, "poses_skipped": 3, "relocalized": 1,
              "max_error_m": math.inf}
    text = M.mcl_text(result)
    back = M.parse_mcl(text)
    assert M.mcl_text(back) == text and back["rows"][0] == rows[0] and back["ticks"] == 2 and back["max_error_m"] == math.inf
    assert math.isnan(back["rows"][1]["est_x"]) and back["rows"][1]["lost"] == 1
    for broken in ("", "something else\n", text.replace("ticks\t2", "tocks\t2"), text.replace("\t2048\t1\t0\t0\n", "\t2048\t1\t0\n")):
        with pytest.raises(ValueError):
            M.parse_mcl(broken)


def test_run_key_is_checked_before_the_fusion_after_scan():
    """tsdf.esdf.mcl in `fuse_from_config` (no GPU, no library: the namespace has no `video`, so reaching the fusion is
    an AttributeError): good values reach the fusion, a bad value or an unknown key is refused before it, a bad scan key
    is reported first, and a switched-off key is not looked at."""
    import types
    from go_slam_amd import tsdf

    def run(mcl_cfg, scan_cfg=None):
        esdf = {"enable": True, "max_distance": 1.0, "mcl": mcl_cfg, **({} if scan_cfg is None else {"scan": scan_cfg})}
        slam = types.SimpleNamespace(cfg={"mode": "rgbd", "tsdf": {"enable": True, "voxel_size": 0.1, "bound": [[-1, 1]] * 3,
                                                                  "esdf": esdf}}, output="/nonexistent/out", mode="rgbd")
        return tsdf.fuse_from_config(slam, stream=(), c2w_list=[], stats={})
    good = {"up_axis": 2, "height": [3.0, 3.6], "beams": 48, "fov_deg": 270.0, "max_range": 3.0, "every": 2, "particles": 256,
            "headings": 72, "drift": {"scale": 1.02, "yaw_deg_per_m": 1.0}, "seed": 1}
    with pytest.raises(AttributeError, match="video"):
        run(good)
    with pytest.raises(AttributeError, match="video"):
        run({"enable": False, "particles": 0})
    for key, value in (("particles", 0), ("drift", {"scale": -1.0}), ("window_m", 1.0)):
        with pytest.raises(ValueError, match="fuse_from_config: tsdf.esdf.mcl"):
            run({**good, key: value})
    with pytest.raises(ValueError, match="fuse_from_config: tsdf.esdf.scan"):
        run({**good, "particles": 0}, {"up_axis": 2, "height": [3.0, 3.6], "beams": 0})


# ---- the closed loop ----------------------------------------------------------------------------------------------------
def test_reported_odometry_alone_ends_three_cells_off():
    cells, _, rot, _ = loop_tables()
    p = np.array([LOOP_START], dtype=np.int32)
    for t, step in enumerate(LOOP_ROUTE):
        p = R.move(p, rot, np.zeros((1, 3), np.int32), reported(t, step), cells.shape)
    true = loop_truth()[-1]
    off = math.hypot(int(p[0, 0]) - true[0], int(p[0, 1]) - true[1]) / 1000.0
    print("dead reckoning ends", p[0].tolist(), "the truth", true, "cells apart", off)
    assert abs(off - LOOP_DEAD_RECKONED_CELLS) <= 0.01
    assert all(SC.scene()[x // 1000, y // 1000] == 254 for x, y, _ in loop_truth())       # the route stays on free cells


@pytest.mark.parametrize("seed", LOOP_SEEDS)
def test_closed_loop_tracks_within_a_cell(seed):
    """The issue's condition: worst position error at most 1.0 cell, worst heading error at most 5 steps, `lost` (three
    ticks running with the best particle's mean cost above sigma_cells^2 = 4, or nothing standing) never raised.  The
    values this loop gets are LOOP_RECORDED; the GPU loop is held against them."""
    rows = run_restatement_loop(seed)
    worst, turn = max(r[0] for r in rows), max(r[1] for r in rows)
    print(f"seed {seed}: worst position error {worst:.4f} cells, worst heading error {turn:.3f} steps, largest best mean "
          f"cost {max(r[2] for r in rows):.4f}, fewest standing {min(r[3] for r in rows)}, resampled {sum(r[4] for r in rows)}")
    assert worst <= 1.0 and turn <= 5.0
    bad = 0
    for r in rows:
        bad = bad + 1 if r[2] > 4.0 else 0
        assert r[3] > 0 and bad < 3
    assert abs(worst - LOOP_RECORDED[seed][0]) < 0.0015 and abs(turn - LOOP_RECORDED[seed][1]) < 0.015


# ---- the kernels' resources ---------------------------------------------------------------------------------------------
_BUDGET = {"mcl_move_kernel": (64, 0), "mcl_weigh_kernel": (64, 64), "mcl_estimate_kernel": (128, 2048),
           "mcl_resample_kernel": (64, 0)}      # (VGPRs, static LDS bytes) as DESIGN.md section 38 states them


def test_kernel_resource_budget(tmp_path):
    """csrc/mcl.hip compiles for gfx950, uses no scratch, and stays within the VGPRs and static LDS of section 38: the
    one-workgroup estimate runs 1024 threads, which 128 VGPRs still allow; the others run at 8 waves per SIMD."""
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "go_slam_amd", "csrc")
    out = tmp_path / "k.s"
    res = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                          "-fno-gpu-rdc", "-munsafe-fp-atomics", "-I", csrc, "-I", os.path.join(ROOT, "include"),
                          "--cuda-device-only", "-S", os.path.join(csrc, "mcl.hip"), "-o", str(out)],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-2000:]
    asm = open(out).read()
    pat = re.compile(r"\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.name:\s+(\S+)\n(?:.*\n)*?"
                     r"\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)")
    seen = {}
    for m in pat.finditer(asm):
        lds, name, scratch, vgpr = int(m.group(1)), m.group(2), int(m.group(3)), int(m.group(4))
        for key, (max_vgpr, max_lds) in _BUDGET.items():
            if key in name:
                seen[key] = (vgpr, lds, scratch)
                assert scratch == 0, f"{name}: {scratch} B of scratch"
                assert vgpr <= max_vgpr, f"{name}: {vgpr} VGPRs > {max_vgpr}"
                assert lds <= max_lds, f"{name}: {lds} B of static LDS > {max_lds}"
    print("mcl.hip (VGPRs, LDS bytes, scratch):", seen)
    assert set(seen) == set(_BUDGET), (seen, sorted(_BUDGET))
