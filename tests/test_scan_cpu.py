"""The scan restatement (tests/scan_restatement.py) against independent models, and the host side of go_slam_amd/scan.py,
without a GPU: the walk against exact rational geometry and against view gain's walk on a [1,n_u,n_v] lattice, the field
against scipy's exact Euclidean transform and a brute-force minimum, the match against a per-candidate brute force, the
recovery scene of DESIGN.md section 36 (three poses, each the unique minimum, with the scores of its table), the argument
errors, the text round trip, and that none of it touches a device."""
import math
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import scan_restatement as R                                   # noqa: E402
import view_gain_restatement as VG                             # noqa: E402

from go_slam_amd import scan as S                              # noqa: E402

SCENE_POSES = (((10, 8), 5), ((28, 20), 13), ((40, 30), 30))   # (cell, yaw index of 32)
SCENE_SCORES = ((2, 20), (0, 30), (3, 26))                     # (best, second best)
SCENE_BEAMS, SCENE_RANGE, SCENE_R, SCENE_YAWS = 60, 30, 6, 32


def scene():
    """48 x 40 at resolution 1: an occupied border, a wall with a door, two boxes and an unknown corner (written last)."""
    c = np.full((48, 40), 254, dtype=np.uint8)
    c[0, :] = c[-1, :] = 0
    c[:, 0] = c[:, -1] = 0
    c[20, 0:25] = 0
    c[20, 9:13] = 254
    c[30:34, 28:33] = 0
    c[5:9, 30:32] = 0
    c[38:48, 0:12] = 205
    c.setflags(write=False)
    return c


def scene_grid(cells=None):
    return {"cells": scene() if cells is None else cells, "origin": (0.0, 0.0), "resolution": 1.0}


def scene_scan(cell, k):
    """(ranges in cells (NaN without a hit), angles, yaws) of the restatement's scan at `cell`, yaw index k."""
    angles = S.beam_angles(SCENE_BEAMS, 360.0)
    yaws = 2.0 * math.pi * np.arange(SCENE_YAWS) / SCENE_YAWS
    kind, _, range_mc = R.cast(scene(), [cell], S.beam_directions(angles, yaws[k])[None], SCENE_RANGE ** 2, True)
    return np.where(kind[0] == 1, range_mc[0] / 1000.0, np.nan), angles, yaws


def random_map(shape, seed):
    rng = np.random.default_rng(seed)
    return rng.choice(np.array([254, 205, 0], dtype=np.uint8), size=shape)


# ---- the walk -----------------------------------------------------------------------------------------------------------
def ray_meets_square(o, d, c):
    """Does the ray o + t d, t >= 0, meet the closed unit square around cell c?  Exact."""
    t0, t1 = Fraction(0), None
    for a in range(2):
        lo, hi = Fraction(2 * (c[a] - o[a]) - 1, 2), Fraction(2 * (c[a] - o[a]) + 1, 2)
        if d[a] == 0:
            if not lo <= 0 <= hi:
                return False
            continue
        ta, tb = sorted((lo / d[a], hi / d[a]))
        t0 = max(t0, ta)
        t1 = tb if t1 is None else min(t1, tb)
    return t1 is None or t0 <= t1


WALK_DIRS = [(1, 0), (0, 1), (-1, 0), (0, -1), (1, 1), (-1, 1), (1, -1), (-1, -1), (32767, 32767), (32767, 1), (1, 32767),
             (-32767, 2), (3, -7), (-5, -2), (32767, -32766), (2, 1), (1, 2), (-30000, 17), (123, 32767)]


@pytest.mark.parametrize("shape,origin", [((23, 17), (11, 8)), ((23, 17), (0, 0)), ((23, 17), (22, 16)), ((1, 9), (0, 4)),
                                          ((40, 1), (7, 0)), ((1, 1), (0, 0))])
def test_walk_against_exact_geometry(shape, origin):
    for d in WALK_DIRS:
        for range2 in (None, 1, 2, 50):
            cells = R.walk(origin, d, shape, range2)
            assert cells[0] == tuple(origin)
            for a, b in zip(cells, cells[1:]):
                assert abs(a[0] - b[0]) + abs(a[1] - b[1]) == 1                      # consecutive cells share a side
                assert (b[0] - a[0]) * d[0] >= 0 and (b[1] - a[1]) * d[1] >= 0          # and never turn back
            for c in cells:
                assert 0 <= c[0] < shape[0] and 0 <= c[1] < shape[1]
                assert ray_meets_square(origin, d, c), (origin, d, c)
                if range2 is not None:
                    assert (c[0] - origin[0]) ** 2 + (c[1] - origin[1]) ** 2 <= range2
            if range2 is not None and len(cells) > 1:                                # the range only cuts the walk short
                assert cells == R.walk(origin, d, shape, None)[:len(cells)]


def test_walk_ties_go_to_the_lower_axis_and_ends_are_final():
    assert R.walk((2, 2), (1, 1), (6, 6)) == [(2, 2), (3, 2), (3, 3), (4, 3), (4, 4), (5, 4), (5, 5)]
    assert R.walk((2, 2), (-7, -7), (6, 6)) == [(2, 2), (1, 2), (1, 1), (0, 1), (0, 0)]
    assert R.walk((2, 2), (0, 0), (6, 6)) == [] and R.walk((2, 2), (32768, 0), (6, 6)) == []
    assert R.walk((6, 2), (1, 0), (6, 6)) == [] and R.walk((-1, 2), (1, 0), (6, 6)) == []
    assert R.walk((2, 2), (1, 0), (6, 6), 1) == [(2, 2), (3, 2)]
    assert R.walk((2, 2), (1, 1), (6, 6), 1) == [(2, 2), (3, 2)] and R.walk((2, 2), (1, 1), (6, 6), 2)[-1] == (3, 3)


def test_walk_equals_view_gains_walk_on_a_flat_lattice():
    for shape, origin in (((23, 17), (11, 8)), ((9, 30), (0, 29)), ((1, 9), (0, 4))):
        for d in WALK_DIRS + [(0, 0), (40000, 1)]:
            for range2 in (None, 2, 77):
                flat = VG.walk((0,) + tuple(origin), (0,) + tuple(d), (1,) + tuple(shape), range2)
                assert [c[1:] for c in flat] == R.walk(origin, d, shape, range2), (shape, origin, d, range2)


def test_cast_kinds_and_ranges_on_a_corridor():
    cells = np.full((1, 12), 254, dtype=np.uint8)
    cells[0, 9], cells[0, 5] = 0, 205
    dirs = np.array([[[0, 1], [0, -1], [0, 0], [0, 40000], [1, 0]]], dtype=np.int32)
    kind, hit, rng = R.cast(cells, [[0, 2]], dirs, 100, True)
    assert kind.tolist() == [[2, 0, 0, 0, 0]] and hit.tolist() == [[5, -1, -1, -1, -1]] and rng.tolist() == [[3000, -1, -1, -1, -1]]
    kind, hit, rng = R.cast(cells, [[0, 2]], dirs, 100, False)
    assert kind.tolist() == [[1, 0, 0, 0, 0]] and hit.tolist() == [[9, -1, -1, -1, -1]] and rng.tolist() == [[7000, -1, -1, -1, -1]]
    kind, hit, rng = R.cast(cells, [[0, 2]], dirs, 36, False)                        # the wall lies beyond the range
    assert kind.tolist() == [[0, 0, 0, 0, 0]]
    kind, hit, rng = R.cast(cells, [[0, 9], [0, 5], [0, 12]], np.tile(dirs, (3, 1, 1)), 100, True)
    assert kind[:, 0].tolist() == [1, 2, 0] and hit[:, 0].tolist() == [9, 5, -1] and rng[:, 0].tolist() == [0, 0, -1]
    assert R.cast(np.array([[0, 254], [254, 0]], np.uint8), [[0, 1]], [[[-1, 1]]], 8, True)[2].tolist() == [[-1]]
    assert R.cast(np.array([[254, 254], [254, 7]], np.uint8), [[0, 0]], [[[1, 1]]], 8, True)[2].tolist() == [[1414]]


# ---- the field ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (1, 30), (30, 1), (21, 26)])
@pytest.mark.parametrize("radius", [1, 3, 15])
def test_field_against_scipy_and_brute_force(shape, radius):
    from scipy import ndimage
    cap = radius * radius + 1
    for seed, fill in ((1, None), (2, 254), (3, 0), (4, "unknown")):
        cells = random_map(shape, seed) if fill is None else np.full(shape, 254, dtype=np.uint8)
        if fill is None:
            cells[np.random.default_rng(seed).random(shape) < 0.7] = 254               # sparse sites: distances beyond the cap
        elif fill == 0:
            cells[:] = 0
        elif fill == "unknown":
            cells[::2] = 205
        got = R.field(cells, radius)
        site = (cells != 254) & (cells != 205)
        if site.any():
            d2 = np.rint(ndimage.distance_transform_edt(~site) ** 2).astype(np.int64)
            us, vs = np.nonzero(site)
            brute = np.array([[((us - u) ** 2 + (vs - v) ** 2).min() for v in range(shape[1])] for u in range(shape[0])])
            assert np.array_equal(d2, brute)
        else:
            d2 = np.full(shape, cap, dtype=np.int64)
        assert got.dtype == np.uint8 and np.array_equal(got, np.minimum(d2, cap))


# ---- the match ----------------------------------------------------------------------------------------------------------
def brute_match(cost, cells, offsets, window, cap, allow_unknown):
    """Candidate by candidate, the beams of one candidate at once."""
    n_u, n_v = cost.shape
    u0, v0, w_u, w_v = window
    Y = offsets.shape[0]
    score = np.zeros((Y, w_u, w_v), dtype=np.uint32)
    best = None
    for y in range(Y):
        off = offsets[y].astype(np.int64)
        small = (np.abs(off + 0.5) < 32768).all(axis=1)
        for i in range(w_u):
            for j in range(w_v):
                u, v = u0 + i, v0 + j
                if not (cells[u, v] == 254 or (allow_unknown and cells[u, v] == 205)):
                    score[y, i, j] = 0xffffffff
                    continue
                e = off + (u, v)
                inside = small & (e[:, 0] >= 0) & (e[:, 0] < n_u) & (e[:, 1] >= 0) & (e[:, 1] < n_v)
                total = int(cost[e[inside, 0], e[inside, 1]].astype(np.int64).sum()) + cap * int((~inside).sum())
                score[y, i, j] = total
                key = (total, (y * w_u + i) * w_v + j)
                best = key if best is None or key < best else best
    return score, R.NO_BEST if best is None else (best[0] << 32) | best[1]


@pytest.mark.parametrize("allow_unknown", [False, True])
def test_match_against_brute_force(allow_unknown):
    cells = random_map((19, 23), 5)
    cells[np.random.default_rng(6).random(cells.shape) < 0.5] = 254
    cost = R.field(cells, 3)
    rng = np.random.default_rng(7)
    offsets = rng.integers(-12, 13, (3, 9, 2)).astype(np.int32)
    offsets[0, 0] = (40000, 0)
    offsets[1, 1] = (0, -32769)
    offsets[2, 2] = (-32768, 32767)
    for window in ((0, 0, 19, 23), (18, 22, 1, 1), (0, 22, 5, 1), (3, 4, 7, 11)):
        got = R.match(cost, cells, offsets, window, 10, allow_unknown)
        want = brute_match(cost, cells, offsets, window, 10, allow_unknown)
        assert np.array_equal(got[0], want[0]) and got[1] == want[1], window
    none = np.zeros((4, 5), dtype=np.uint8)
    score, best = R.match(R.field(none, 2), none, offsets[:, :2], (0, 0, 4, 5), 5, allow_unknown)
    assert best == R.NO_BEST and (score == 0xffffffff).all()


def test_match_ties_go_to_the_lowest_index():
    room = np.zeros((9, 13), dtype=np.uint8)
    room[1:-1, 1:-1] = 254                                     # an empty rectangular room: half a turn changes nothing
    angles = S.beam_angles(16, 360.0)
    yaws = 2.0 * math.pi * np.arange(4) / 4
    kind, _, range_mc = R.cast(room, [[5, 4]], S.beam_directions(angles, yaws[3])[None], 400, True)
    offsets = S.beam_offsets(range_mc[0] / 1000.0, angles, yaws, 1.0)
    score, best = R.match(R.field(room, 3), room, offsets, (0, 0, 9, 13), 10, False)
    assert score[3, 5, 4] == score[1, 3, 8] == (best >> 32)     # the pose and its mirror image score the same
    assert (best & 0xffffffff) == (1 * 9 + 3) * 13 + 8         # and the lower index wins


# ---- the recovery scene -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", range(len(SCENE_POSES)))
def test_scene_poses_are_recovered_exactly(n):
    (cell, k), (first, second) = SCENE_POSES[n], SCENE_SCORES[n]
    cells = scene()
    ranges, angles, yaws = scene_scan(cell, k)
    offsets = S.beam_offsets(ranges, angles, yaws, 1.0, 0.0, float(SCENE_RANGE))
    score, best = R.match(R.field(cells, SCENE_R), cells, offsets, (0, 0, 48, 40), SCENE_R ** 2 + 1, False)
    index = best & 0xffffffff
    assert (index // (48 * 40), (index // 40) % 48, index % 40) == (k,) + cell
    flat = np.sort(score.reshape(-1).astype(np.int64))
    print(f"scene pose {cell} yaw {k}: best {best >> 32}, second best {flat[1]}")
    assert (best >> 32, int(flat[1])) == (first, second) and flat[0] == first


# ---- the host side ------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_device(monkeypatch):
    """Any use of the library or of a device fails the test."""
    from go_slam_amd import _lib

    def refuse(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(_lib, "lib", refuse)
    monkeypatch.setattr(_lib, "stream_ptr", refuse)
    monkeypatch.setattr(torch.Tensor, "to", refuse)
    monkeypatch.setattr(torch.Tensor, "cuda", refuse)


def test_beams_on_the_host(no_device):
    a = S.beam_angles(8, 360.0)
    assert a.dtype == np.float64 and np.array_equal(a, -math.pi + np.arange(8) * (2.0 * math.pi / 8))
    assert np.allclose(S.beam_angles(5, 180.0), np.radians([-90, -45, 0, 45, 90])) and S.beam_angles(1, 90.0).tolist() == [0.0]
    d = S.beam_directions([0.0, math.pi / 2, math.pi, math.pi / 4], 0.0)
    assert d.dtype == np.int32 and d.tolist() == [[32767, 0], [0, 32767], [-32767, 0], [32767, 32767]]
    assert S.beam_directions([0.0], math.pi / 2).tolist() == [[0, 32767]]               # a positive yaw turns toward +v
    assert S.beam_directions([0.0, 1.0], [0.0, 0.5, 1.0]).shape == (3, 2, 2)
    assert np.abs(S.beam_directions(S.beam_angles(360), 0.3)).max(axis=-1).tolist() == [32767] * 360
    r = np.array([1.0, np.nan, 2.5, np.inf, 0.05, 9.0])
    ang = np.array([0.0, 0.1, math.pi / 2, 0.2, 0.3, math.pi])
    assert S.valid_beams(r, 0.1, 8.0).tolist() == [True, False, True, False, False, False]
    off = S.beam_offsets(r, ang, [0.0, math.pi / 2], 0.5, 0.1, 8.0)
    assert off.dtype == np.int32 and off.tolist() == [[[2, 0], [0, 5]], [[0, 2], [-5, 0]]]
    assert S.beam_offsets([np.nan], [0.0], [0.0], 1.0).shape == (1, 0, 2)
    want = np.floor(np.array(2.5) * np.cos(np.array(0.3) + np.array(1.1)) / 0.07 + 0.5)
    assert S.beam_offsets([2.5], [0.3], [1.1], 0.07)[0, 0, 0] == int(want)
    for call in (lambda: S.beam_angles(0), lambda: S.beam_angles(4097), lambda: S.beam_angles(4, 0.0),
                 lambda: S.beam_angles(4, 361.0), lambda: S.beam_angles(True), lambda: S.beam_directions([[0.0]], 0.0),
                 lambda: S.beam_directions([math.nan], 0.0), lambda: S.beam_directions([0.0], math.inf),
                 lambda: S.beam_offsets([1.0, 2.0], [0.0], [0.0], 1.0), lambda: S.beam_offsets([1.0], [0.0], [0.0], 0.0),
                 lambda: S.beam_offsets([1.0], [0.0], [0.0], 1.0, 2.0, 1.0), lambda: S.beam_offsets([1.0], [0.0], [[0.0]], 1.0)):
        with pytest.raises(ValueError):
            call()


def test_argument_errors_come_before_the_device(no_device):
    grid = scene_grid()
    cells = torch.from_numpy(np.array(scene()))
    angles = S.beam_angles(8)
    ranges = np.full(8, 3.0)
    bad = [
        lambda: S.scan_on_map({"cells": scene()}, (5.5, 5.5), 0.0),
        lambda: S.scan_on_map(grid, (50.0, 5.0), 0.0),                               # outside the map
        lambda: S.scan_on_map(grid, (5.0, math.nan), 0.0),
        lambda: S.scan_on_map(grid, (5.0, 5.0), [0.0, 1.0]),
        lambda: S.scan_on_map(grid, [[5.0, 5.0]], 0.0),
        lambda: S.scan_on_map(grid, (5.0, 5.0), 0.0, n_beams=0),
        lambda: S.scan_on_map(grid, (5.0, 5.0), 0.0, fov_deg=400.0),
        lambda: S.scan_on_map(grid, (5.0, 5.0), 0.0, max_range=0.0),
        lambda: S.scan_on_map(grid, (5.0, 5.0), 0.0, stop_unknown=1),
        lambda: S.scan_on_map(scene_grid(np.zeros((3, 1025), np.uint8)), (0.5, 0.5), 0.0),
        lambda: S.scan_on_map(scene_grid(np.zeros((3, 4), np.int32)), (0.5, 0.5), 0.0),
        lambda: S.scan_on_map({**grid, "resolution": 0.0}, (0.5, 0.5), 0.0),
        lambda: S.cost_field(grid, 0), lambda: S.cost_field(grid, 16), lambda: S.cost_field(grid, 2.0),
        lambda: S.match_scan(grid, ranges, angles, [0.0], window=(0, 0, 49, 1)),
        lambda: S.match_scan(grid, ranges, angles, [0.0], window=(48, 0, 1, 1)),
        lambda: S.match_scan(grid, ranges, angles, [0.0], window=(0, 0, 0, 1)),
        lambda: S.match_scan(grid, ranges, angles, [0.0], window=(0, 0, 1)),
        lambda: S.match_scan(grid, ranges[:7], angles, [0.0]),
        lambda: S.match_scan(grid, np.full(8, np.nan), angles, [0.0]),                # no valid beam
        lambda: S.match_scan(grid, ranges, angles, np.zeros(1025)),
        lambda: S.match_scan(grid, ranges, angles, [0.0], radius_cells=16),
        lambda: S.match_scan(grid, ranges, angles, [0.0], allow_unknown=1),
        lambda: S.match_scan(grid, ranges, angles, [0.0], min_range=-1.0),
        lambda: S.localize_on_map(grid, ranges, angles, n_yaw=0),
        lambda: S.localize_on_map(grid, ranges, angles, n_yaw=1025),
        lambda: S.localize_on_map(grid, ranges, angles, around=(1, 2, 3)),
        lambda: S.localize_on_map(grid, ranges, angles, around=((60.0, 5.0), 1.0, None, None)),
        lambda: S.localize_on_map(grid, ranges, angles, around=((6.0, 5.0), -1.0, None, None)),
        lambda: S.localize_on_map(grid, ranges, angles, around=(None, None, 0.0, -0.1)),
        lambda: S.localize_on_map(grid, ranges, angles, tol_cells=-1),
        lambda: S.cast(cells, [[1, 1]], [[[1, 0]]], 0), lambda: S.cast(cells, [[1, 1]], [[[1, 0]]], S.MAX_RANGE2 + 1),
        lambda: S.cast(cells.int(), [[1, 1]], [[[1, 0]]], 4), lambda: S.cast(cells, [[1, 1]], [[[1, 0]]], 4, stop_unknown=0),
        lambda: S.cast(cells, [[1, 1]], [[[1, 0]]], 4),                               # a host tensor: there is no host path
        lambda: S.field(cells, 0), lambda: S.field(cells[None], 3), lambda: S.field(cells, 3),
        lambda: S.match(cells, cells[:, :5], [[[0, 0]]], None, 10), lambda: S.match(cells, cells, [[[0, 0]]], None, 0),
        lambda: S.match(cells, cells, [[[0, 0]]], None, 227), lambda: S.match(cells, cells, [[[0, 0]]], None, 10),
    ]
    for n, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"call {n} raised nothing")
    with pytest.raises(ValueError, match="outside the map"):
        S.scan_on_map(grid, (50.0, 5.0), 0.0)
    assert S.localize_on_map(grid, np.full(8, np.nan), angles)["found"] is False       # no valid beam: no launch


def test_around_restricts_window_and_yaws(no_device):
    window, ks = S._around(((10.5, 8.5), 3.0, math.pi / 2, 0.2), 32, (48, 40), [0.0, 0.0], 1.0, "t")
    assert window == (7, 5, 7, 7) and ks.tolist() == [7, 8, 9]
    window, ks = S._around(((0.5, 39.5), 2.5, None, None), 32, (48, 40), [0.0, 0.0], 1.0, "t")
    assert window == (0, 36, 4, 4) and ks.tolist() == list(range(32))
    window, ks = S._around((None, None, -0.01, 0.3), 32, (48, 40), [0.0, 0.0], 1.0, "t")
    assert window is None and ks.tolist() == [0, 1, 31]
    assert S._around((None, None, 0.09, 0.0), 32, (48, 40), [0.0, 0.0], 1.0, "t")[1].tolist() == [0]


def test_config_and_text_round_trip(no_device):
    assert S.scan_config(None) is None and S.scan_config({"enable": False}) is None
    cfg = S.scan_config({"up_axis": 1, "height": [-0.2, 0.4]})
    assert cfg == {"up_axis": 1, "height": (-0.2, 0.4), "beams": 360, "fov_deg": 360.0, "max_range": None, "every": 5,
                   "n_yaw": 360, "window_m": 1.0}
    for bad in ({"up_axis": 1}, {"up_axis": 3, "height": [0, 1]}, {"up_axis": 1, "height": [1, 0]},
                {"up_axis": 1, "height": [0, 1], "beam": 3}, {"up_axis": 1, "height": [0, 1], "beams": 0},
                {"up_axis": 1, "height": [0, 1], "every": 0}, {"up_axis": 1, "height": [0, 1], "n_yaw": 2000},
                {"up_axis": 1, "height": [0, 1], "window_m": -1.0}, {"up_axis": 1, "height": [0, 1], "max_range": 0.0},
                {"up_axis": 1, "height": [0, 1], "enable": 1}, [1, 2]):
        with pytest.raises(ValueError, match="tsdf.esdf.scan"):
            S.scan_config(bad)
    rows = [{"true_u": 3, "true_v": 4, "true_yaw": 0.1 + 0.2, "true_yaw_index": 17, "found_u": 3, "found_v": 5,
             "found_yaw_index": 18, "score": 41, "inlier_fraction": 1.0 / 3.0},
            {"true_u": 0, "true_v": 0, "true_yaw": -math.pi, "true_yaw_index": 180, "found_u": -1, "found_v": -1,
             "found_yaw_index": -1, "score": -1, "inlier_fraction": 0.0}]
    result = {"n_yaw": 360, "poses_tried": 2, "poses_skipped": 7, "poses_recovered": 1, "rows": rows}
    text = S.scan_localize_text(result)
    assert S.parse_scan_localize(text) == result and S.scan_localize_text(S.parse_scan_localize(text)) == text
    empty = {"n_yaw": 8, "poses_tried": 0, "poses_skipped": 0, "poses_recovered": 0, "rows": []}
    assert S.parse_scan_localize(S.scan_localize_text(empty)) == empty
    with pytest.raises(ValueError):
        S.parse_scan_localize("something else\n")
    poses = S.planar_poses([torch.eye(4), torch.tensor([[0.0, 0, 1, 2], [0, 1, 0, 3], [-1, 0, 0, 4], [0, 0, 0, 1]])], (0, 2))
    assert poses[0] == ((0.0, 0.0), math.pi / 2) and poses[1] == ((2.0, 4.0), 0.0)
    assert S.planar_poses([torch.eye(4)], (0, 1)) == [None]                               # looks along the up axis
    assert S.count_inliers([1, 1, 2, 0, 1], [3000, 5000, 3000, -1, 900], [3.0, 3.0, 3.0, 3.0, 3.0], 2) == 2
