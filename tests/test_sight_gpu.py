"""Line of sight and the straightened path on the MI355X (csrc/sight.hip, go_slam_amd/plan.py, ESDF.sees / straighten):
every result equals the serial restatement (tests/sight_restatement.py) with torch.equal -- the segments from the centre
of a 13^3 lattice to every cell, the sight matrix and the programme on a random lattice's path, on a serpentine's and at
the smallest sizes, for windows on both sides of the ballot's word boundary; the C entries' refusals; the hand-built room
with a door planned through end to end; and an only-tracking run with tsdf.esdf.plan.straighten ends with
map/path_straight.txt."""
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import sight_restatement as SR                                 # noqa: E402
import test_esdf_gpu as EG                                     # noqa: E402  (its only-tracking run)
import test_geodesic_gpu as GG                                 # noqa: E402  (the serpentine and the room with a door)
import test_sight_cpu as SC                                    # noqa: E402  (the lattices and their paths)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INVALID = -1
room = GG.room                                              # the module-scoped fixture, built once here too
_REF = {}
PLAN_KEYS = {"reachable", "cells", "points", "length_m", "min_clearance_m", "start_cell", "goal_cell", "sweeps"}
WAY_KEYS = {"waypoint_index", "waypoints", "waypoint_points", "straight_length_m"}


def gpu(a):
    return torch.from_numpy(np.array(a)).to(DEV)             # a copy: the shared references are read-only


def full_matrix(name, passable, cells):
    """The restatement's sight matrix at the widest window, once per named path."""
    key = (name, "matrix")
    if key not in _REF:
        _REF[key] = SR.sight_matrix(passable, cells, max(len(cells) - 1, 1))
        _REF[key].setflags(write=False)
    return _REF[key]


def cut(matrix, window):
    """The matrix of a narrower window: bit b of a row does not depend on the window, bits at and beyond it are 0."""
    words = (window + 63) // 64
    out = matrix[:, :words].copy()
    if window % 64:
        out[:, -1] &= np.uint64((1 << (window % 64)) - 1)
    return out


def as_u64(t):
    return t.cpu().numpy().view(np.uint64)


def run_path(passable, cells, window):
    """(sight int64 [L,words], index int32 [L] pre-filled with -7, n_out, length) straight from the C entries."""
    from go_slam_amd import _lib
    L, P = _lib.lib(), _lib.ptr
    p = gpu(passable).to(torch.uint8)
    c = gpu(np.asarray(cells, dtype=np.int32).reshape(-1, 3))
    n = int(c.shape[0])
    sight = torch.full((n, (window + 63) // 64), -1, dtype=torch.int64, device=DEV)
    index = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    tail = torch.full((2,), -7, dtype=torch.int32, device=DEV)
    stream = _lib.stream_ptr(DEV)
    assert L.gs_path_sight(P(p), *p.shape, P(c), n, window, P(sight), stream) == 0
    assert L.gs_path_shortcut(P(sight), P(c), n, window, P(index), P(tail[0:]), P(tail[1:]), stream) == 0
    k, length = tail.cpu().tolist()
    return sight, index.cpu().numpy(), k, length


def assert_shortcut(matrix, cells, window, index, k, length):
    """index, n_out and length against the restatement's programme on `matrix`; what is not written holds -7."""
    w_index, w_length = SR.shortcut(matrix, cells, window)
    if w_index is None:
        assert (k, length) == (-1, -7) and (index == -7).all()
    else:
        assert k == len(w_index) and length == w_length and np.array_equal(index[:k], w_index)
        assert (index[k:] == -7).all()


def assert_path(name, passable, cells, window):
    sight, index, k, length = run_path(passable, cells, window)
    want = cut(full_matrix(name, passable, cells), window)
    assert np.array_equal(as_u64(sight), want), (name, window)
    assert_shortcut(want, cells, window, index, k, length)
    return index[:k], length


# ---- segments ---------------------------------------------------------------------------------------------------------------
def test_segments_from_the_centre_to_every_cell(built_lib):
    from go_slam_amd import plan
    rng = np.random.default_rng(5)
    dims = (13, 13, 13)
    passable = rng.random(dims) >= 0.10
    passable[6, 6, 6] = True
    field = rng.integers(-20, 20, dims).astype(np.int32)
    b = np.array(list(np.ndindex(*dims)), dtype=np.int32)
    outside = np.array([[13, 6, 6], [6, -1, 6], [6, 6, 13], [-1, -1, -1]], dtype=np.int32)
    b = np.concatenate([b, outside])
    a = np.tile(np.array([[6, 6, 6]], dtype=np.int32), (len(b), 1))
    a, b = np.concatenate([a, outside]), np.concatenate([b, np.tile([[6, 6, 6]], (4, 1)).astype(np.int32)])
    assert len(a) == 2197 + 8
    want = np.array([SR.sees(passable, a[i], b[i]) for i in range(len(a))])
    print("segments", len(a), "clear", int(want.sum()))
    assert want[:2197].any() and not want[:2197].all() and not want[2197:].any() and want[6 * 169 + 6 * 13 + 6]
    got = plan.line_of_sight(gpu(passable), a, b)
    assert got.dtype == torch.bool and torch.equal(got.cpu(), torch.from_numpy(want))
    assert torch.equal(plan.line_of_sight(gpu(passable), gpu(b), gpu(a).long()).cpu(), torch.from_numpy(want))   # symmetric
    mins = [SR.segment_min(field, a[i], b[i]) for i in range(len(a))]
    tied = sum(1 for i in range(2197) if sum(1 for c in SR.walk(a[i], b[i]) if field[c] == mins[i][0]) > 1)
    print("segments whose minimum is held by several cells", tied)
    assert tied > 100 and mins[-1] == (-2 ** 31, -1)
    value, cell = plan.segment_min(gpu(field), a, b)
    assert value.dtype == cell.dtype == torch.int32
    assert torch.equal(value.cpu(), torch.tensor([m[0] for m in mins], dtype=torch.int32))
    assert torch.equal(cell.cpu(), torch.tensor([m[1] for m in mins], dtype=torch.int32))
    none = plan.line_of_sight(gpu(passable), np.zeros((0, 3), dtype=np.int32), [])
    assert tuple(none.shape) == (0,)


# ---- the sight matrix and the programme -------------------------------------------------------------------------------
@pytest.mark.parametrize("window", [1, 4, 63, 64, 65, "L-1"])
def test_random_lattice_path_equals_the_restatement(built_lib, window):
    passable, cost, cells = SC.random_case()
    L = len(cells)
    window = L - 1 if window == "L-1" else window
    index, length = assert_path("random", passable, cells, window)
    assert index[0] == 0 and index[-1] == L - 1 and length <= int(cost[tuple(cells[0])])
    if window == 1:
        assert len(index) == L and length == int(cost[tuple(cells[0])])
    if window == L - 1:
        assert (length, len(index)) == (74566, 15)
        again = run_path(passable, cells, window)            # the same bits a second time
        first = run_path(passable, cells, window)
        assert torch.equal(again[0], first[0]) and np.array_equal(again[1], first[1]) and again[2:] == first[2:]


@pytest.mark.parametrize("window", [64, 128, 129, "L-1"])
def test_serpentine_path_equals_the_restatement(built_lib, window):
    passable, cost, cells = SC.lattice_path("serpentine", GG.serpentine(), (1, 0, 0))
    L = len(cells)
    assert L > 400                                          # several words per row, and rows shorter than the window
    window = L - 1 if window == "L-1" else window
    index, length = assert_path("serpentine", passable, cells, window)
    print("serpentine: L", L, "window", window, "kept", len(index), "length", length, "lattice", int(cost[tuple(cells[0])]))
    assert len(index) < L // 8 and length < int(cost[tuple(cells[0])])


def test_smallest_paths_and_lattices(built_lib):
    from go_slam_amd import plan
    one = np.ones((1, 1, 1), dtype=bool)
    sight, index, k, length = run_path(one, [[0, 0, 0]], 1)
    assert as_u64(sight).tolist() == [[0]] and (k, length) == (1, 0) and index.tolist() == [0]
    res = plan.straighten(gpu(one), [[0, 0, 0]])
    assert res["index"].tolist() == [0] and res["cells"].tolist() == [[0, 0, 0]] and res["length"] == 0
    assert res["window"] == 1
    two = np.ones((1, 1, 2), dtype=bool)
    sight, index, k, length = run_path(two, [[0, 0, 0], [0, 0, 1]], 1)
    assert as_u64(sight).tolist() == [[0], [1]] and (k, length) == (2, 1000) and index.tolist() == [0, 1]
    sight, index, k, length = run_path(two, [[0, 0, 0], [0, 0, 0]], 1)     # a cell twice: a leg of no length
    assert as_u64(sight).tolist() == [[0], [1]] and (k, length) == (2, 0)
    passable, cost, cells = SC.two_rooms_case()             # [1,n,n]
    for window in (1, 4, 16, len(cells) - 1):
        index, length = assert_path("two rooms", passable, cells, window)
        res = plan.straighten(gpu(passable), cells, window)
        assert res["index"].dtype == torch.int32 and res["index"].is_cuda and res["window"] == window
        assert np.array_equal(res["index"].cpu().numpy(), index) and res["length"] == length
        assert np.array_equal(res["cells"].cpu().numpy(), cells[index])
    wide = plan.straighten(gpu(passable), torch.from_numpy(np.array(cells)), 10 ** 6)       # cut to L - 1
    assert wide["window"] == len(cells) - 1 and wide["length"] == length


def test_blocked_cells_in_the_path(built_lib):
    from go_slam_amd import plan
    passable, cost, cells = SC.random_case()
    L = len(cells)
    gone = np.argwhere(~passable)[0]
    middle = np.array(cells)
    middle[L // 2] = gone
    sight, index, k, length = run_path(passable, middle, L - 1)
    want = SR.sight_matrix(passable, middle, L - 1)
    assert np.array_equal(as_u64(sight), want)
    assert not want[L // 2].any() and not any(int(want[j, (j - 1 - L // 2) // 64]) >> ((j - 1 - L // 2) % 64) & 1
                                              for j in range(L // 2 + 1, L))
    assert_shortcut(want, middle, L - 1, index, k, length)
    assert k > 2 and L // 2 not in index[:k]
    middle[3] = [9, 0, 0]                                   # and one outside the lattice
    sight, index, k, length = run_path(passable, middle, 5)
    want = SR.sight_matrix(passable, middle, 5)
    assert np.array_equal(as_u64(sight), want)
    assert_shortcut(want, middle, 5, index, k, length)
    last = np.array(cells)
    last[-1] = gone
    sight, index, k, length = run_path(passable, last, L - 1)
    assert k == -1 and length == -7 and (index == -7).all()  # n_out alone was written
    assert SR.straighten(passable, last, L - 1) == (None, None)
    with pytest.raises(RuntimeError, match="cannot be reached"):
        plan.straighten(gpu(passable), last)
    torch.cuda.synchronize()
    assert plan.straighten(gpu(passable), cells)["length"] == 74566          # the device is fine afterwards


def test_c_abi_refusals_leave_the_outputs_untouched(built_lib):
    from go_slam_amd import _lib
    L, P = _lib.lib(), _lib.ptr
    stream = _lib.stream_ptr(DEV)
    dims = (9, 11, 70)
    passable = torch.ones(dims, dtype=torch.uint8, device=DEV)
    field = torch.zeros(dims, dtype=torch.int32, device=DEV)
    segs = torch.zeros((4, 6), dtype=torch.int32, device=DEV)
    out = torch.full((4,), 7, dtype=torch.uint8, device=DEV)
    value = torch.full((4,), -7, dtype=torch.int32, device=DEV)
    cell = torch.full((4,), -7, dtype=torch.int32, device=DEV)
    cells = torch.zeros((8, 3), dtype=torch.int32, device=DEV)
    sight = torch.full((8, 1), -1, dtype=torch.int64, device=DEV)
    index = torch.full((8,), -7, dtype=torch.int32, device=DEV)
    tail = torch.full((2,), -7, dtype=torch.int32, device=DEV)
    for bad in ((0, 11, 70), (9, 1025, 70), (9, 11, -1)):
        assert L.gs_segment_sight(P(passable), *bad, P(segs), 4, P(out), stream) == INVALID
        assert L.gs_segment_min(P(field), *bad, P(segs), 4, P(value), P(cell), stream) == INVALID
        assert L.gs_path_sight(P(passable), *bad, P(cells), 8, 7, P(sight), stream) == INVALID
    assert L.gs_segment_sight(None, *dims, P(segs), 4, P(out), stream) == INVALID
    assert L.gs_segment_sight(P(passable), *dims, None, 4, P(out), stream) == INVALID
    assert L.gs_segment_sight(P(passable), *dims, P(segs), 4, None, stream) == INVALID
    assert L.gs_segment_sight(P(passable), *dims, P(segs), -1, P(out), stream) == INVALID
    assert L.gs_segment_min(None, *dims, P(segs), 4, P(value), P(cell), stream) == INVALID
    assert L.gs_segment_min(P(field), *dims, None, 4, P(value), P(cell), stream) == INVALID
    assert L.gs_segment_min(P(field), *dims, P(segs), 4, None, P(cell), stream) == INVALID
    assert L.gs_segment_min(P(field), *dims, P(segs), 4, P(value), None, stream) == INVALID
    assert L.gs_segment_min(P(field), *dims, P(segs), -1, P(value), P(cell), stream) == INVALID
    assert L.gs_path_sight(None, *dims, P(cells), 8, 7, P(sight), stream) == INVALID
    assert L.gs_path_sight(P(passable), *dims, None, 8, 7, P(sight), stream) == INVALID
    assert L.gs_path_sight(P(passable), *dims, P(cells), 8, 7, None, stream) == INVALID
    for n, w in ((0, 1), (-3, 1), (SR.MAX_CELLS + 1, 256), (8, 0), (8, 8), (8, -1), (1, 2), (1, 0)):
        assert L.gs_path_sight(P(passable), *dims, P(cells), n, w, P(sight), stream) == INVALID, (n, w)
        assert L.gs_path_shortcut(P(sight), P(cells), n, w, P(index), P(tail[0:]), P(tail[1:]), stream) == INVALID, (n, w)
    assert L.gs_path_shortcut(None, P(cells), 8, 7, P(index), P(tail[0:]), P(tail[1:]), stream) == INVALID
    assert L.gs_path_shortcut(P(sight), None, 8, 7, P(index), P(tail[0:]), P(tail[1:]), stream) == INVALID
    assert L.gs_path_shortcut(P(sight), P(cells), 8, 7, None, P(tail[0:]), P(tail[1:]), stream) == INVALID
    assert L.gs_path_shortcut(P(sight), P(cells), 8, 7, P(index), None, P(tail[1:]), stream) == INVALID
    assert L.gs_path_shortcut(P(sight), P(cells), 8, 7, P(index), P(tail[0:]), None, stream) == INVALID
    assert b"path_shortcut" in L.gs_last_error()
    torch.cuda.synchronize()
    assert (out == 7).all() and (value == -7).all() and (cell == -7).all() and (sight == -1).all()
    assert (index == -7).all() and (tail == -7).all()        # nothing was launched
    assert L.gs_segment_sight(P(passable), *dims, P(segs), 0, P(out), stream) == 0 and (out == 7).all()
    assert L.gs_path_sight(P(passable), *dims, P(cells), 8, 7, P(sight), stream) == 0
    assert as_u64(sight)[:, 0].tolist() == [(1 << j) - 1 for j in range(8)]          # one cell eight times sees itself


# ---- end to end on the hand-built room --------------------------------------------------------------------------------
VOXEL, START, GOAL = GG.VOXEL, GG.START, GG.GOAL


def test_plan_straightens_through_the_door_and_equals_the_restatement(room):
    from go_slam_amd import _lib, plan
    vol, field = room
    radius = VOXEL
    with _lib.kernel_timer(DEV) as timer:
        plain = field.plan(START, GOAL, robot_radius=radius)
        torch.cuda.synchronize()
    launched = set(timer.read())
    assert set(plain) == PLAN_KEYS and "geodesic_path" in launched            # the dict and the launches of before
    assert not launched & {"segment_sight", "segment_min", "path_sight", "path_shortcut"}
    res = field.plan(START, GOAL, robot_radius=radius, straighten=True)
    assert set(res) == PLAN_KEYS | WAY_KEYS | {"straight_min_clearance_m"}
    assert torch.equal(res["cells"], plain["cells"]) and res["length_m"] == plain["length_m"]
    p = field.passable(radius).cpu().numpy() != 0
    cells = res["cells"].cpu().numpy()
    L = len(cells)
    index = res["waypoint_index"].cpu().numpy()
    way = res["waypoints"].cpu().numpy()
    print("cells", L, "waypoints", len(index), "length_m", res["length_m"], "straight", res["straight_length_m"],
          "clearance", res["min_clearance_m"], "straight", res["straight_min_clearance_m"])
    assert index[0] == 0 and index[-1] == L - 1 and len(index) < L and np.array_equal(way, cells[index])
    assert way[0].tolist() == res["start_cell"] and way[-1].tolist() == res["goal_cell"]
    assert res["straight_length_m"] <= res["length_m"]
    assert all(SR.sees(p, way[i], way[i + 1]) for i in range(len(way) - 1))
    w_index, w_length = SR.straighten(p, cells, 256)
    assert np.array_equal(index, w_index) and res["straight_length_m"] == w_length * VOXEL / 1000.0
    assert res["waypoint_points"].dtype == torch.float64
    assert np.array_equal(res["waypoint_points"].cpu().numpy(), way.astype(np.float64) * VOXEL)      # lo = 0
    d2 = field.d2.cpu().numpy()
    worst = min(SR.segment_min(d2, way[i], way[i + 1]) for i in range(len(way) - 1))
    assert res["straight_min_clearance_m"] == float(field.dist.cpu().numpy().reshape(-1)[worst[1]])
    assert res["straight_min_clearance_m"] > radius          # every crossed cell passes: d2 >= 2 voxels^2
    later = field.straighten(plain, robot_radius=radius)     # the same from the finished dict; `plain` is not changed
    assert set(plain) == PLAN_KEYS and torch.equal(later["waypoint_index"], res["waypoint_index"])
    assert later["straight_length_m"] == res["straight_length_m"]
    assert later["straight_min_clearance_m"] == res["straight_min_clearance_m"]
    narrow = field.plan(START, GOAL, robot_radius=radius, straighten=True, window=1)
    assert len(narrow["waypoint_index"]) == L and narrow["straight_length_m"] == res["length_m"]
    # a goal the start does not see: the route bends at the door
    far_goal = (33 * VOXEL, 16 * VOXEL, 34 * VOXEL)
    assert field.sees(START, far_goal, robot_radius=radius).cpu().tolist() == [False]
    bent = field.plan(START, far_goal, robot_radius=radius, straighten=True)
    cells = bent["cells"].cpu().numpy()
    index = bent["waypoint_index"].cpu().numpy()
    w_index, w_length = SR.straighten(p, cells, 256)
    print("bent: cells", len(cells), "waypoints", index.tolist(), "length_m", bent["length_m"], "straight",
          bent["straight_length_m"])
    assert 2 < len(index) < len(cells) and np.array_equal(index, w_index)
    assert bent["straight_length_m"] == w_length * VOXEL / 1000.0 < bent["length_m"]


def test_sees_is_false_across_the_wall_and_true_through_the_door(room):
    vol, field = room
    a = np.array([[8, 6, 30], [10, 8, 20], [8, 6, 30], [8, 6, 30]], dtype=np.float64) * VOXEL
    b = np.array([[33, 6, 30], [30, 8, 20], [8, 6, 31], [80, 6, 30]], dtype=np.float64) * VOXEL
    got = field.sees(a, b, robot_radius=VOXEL)
    p = field.passable(VOXEL).cpu().numpy() != 0
    want = [SR.sees(p, (a[i] / VOXEL).astype(int), (b[i] / VOXEL).astype(int)) for i in range(4)]
    assert got.dtype == torch.bool and got.cpu().tolist() == want == [False, True, True, False]
    assert field.sees(a[1], torch.from_numpy(b[1]), robot_radius=VOXEL).cpu().tolist() == [True]
    assert field.sees(a[1], b[1], robot_radius=4 * VOXEL).cpu().tolist() == [False]          # wider than the door


def test_a_robot_wider_than_the_door_has_no_waypoints(room):
    vol, field = room
    res = field.plan(START, GOAL, robot_radius=4 * VOXEL, straighten=True)
    assert res["reachable"] is False and res["cells"].shape[0] == 0 and res["length_m"] == math.inf
    assert tuple(res["waypoint_index"].shape) == (0,) and res["waypoint_index"].dtype == torch.int32
    assert tuple(res["waypoints"].shape) == (0, 3) and tuple(res["waypoint_points"].shape) == (0, 3)
    assert res["straight_length_m"] == math.inf and math.isnan(res["straight_min_clearance_m"])
    assert set(res) == PLAN_KEYS | WAY_KEYS | {"straight_min_clearance_m"}


def test_plan_on_map_straightens_on_the_slice(room):
    from go_slam_amd import plan
    vol, field = room
    grid = field.occupancy_slice(1, (6 * VOXEL, 8 * VOXEL), robot_radius=VOXEL)
    ends = (START[0], START[2]), (GOAL[0], GOAL[2])
    plain = plan.plan_on_map(grid, *ends)
    assert set(plain) == PLAN_KEYS - {"min_clearance_m"}
    res = plan.plan_on_map(grid, *ends, straighten=True)
    assert set(res) == (PLAN_KEYS - {"min_clearance_m"}) | WAY_KEYS and torch.equal(res["cells"], plain["cells"])
    cells = res["cells"].cpu().numpy()
    free = (grid["cells"].cpu().numpy() == 254)[None]
    cells3 = np.concatenate([np.zeros((len(cells), 1), dtype=cells.dtype), cells], axis=1)
    w_index, w_length = SR.straighten(free, cells3, 256)
    index = res["waypoint_index"].cpu().numpy()
    assert np.array_equal(index, w_index) and 2 <= len(index) < len(cells)
    assert res["straight_length_m"] == w_length * VOXEL / 1000.0 <= res["length_m"]
    way = res["waypoints"].cpu().numpy()
    assert way.shape == (len(index), 2) and np.array_equal(way, cells[index])
    centres = np.array(grid["origin"]) + (way.astype(np.float64) + 0.5) * VOXEL
    assert np.array_equal(res["waypoint_points"].cpu().numpy(), centres)


# ---- whole run ------------------------------------------------------------------------------------------------------
def test_only_tracking_run_ends_with_a_straightened_path_file(built_lib, tmp_path, monkeypatch):
    from go_slam_amd import plan
    from go_slam_amd.slam import SLAM
    returned = []
    terminate = SLAM.terminate

    def keeping(self, *args, **kw):
        returned.append(terminate(self, *args, **kw))
        return returned[-1]
    monkeypatch.setattr(SLAM, "terminate", keeping)
    plan_cfg = {"enable": True, "robot_radius": 0.2, "snap": 1.0, "allow_unknown": True, "goal": [0.6, 0.0, 0.3]}

    def cfg(plan_cfg):
        return {"enable": True, "source": "sensor", "voxel_size": 0.1,
                "esdf": {"enable": True, "max_distance": 1.0, "plan": plan_cfg}}
    with_dir, without_dir = str(tmp_path / "with"), str(tmp_path / "without")
    EG.TG.whole_run(with_dir, cfg({**plan_cfg, "straighten": {"enable": True, "window": 128}}))
    stats = returned[0]
    head, points = plan.parse_straight_path(open(f"{with_dir}/map/path_straight.txt").read())
    lattice, lattice_points = plan.parse_path(open(f"{with_dir}/map/path.txt").read())
    print("map/path_straight.txt:", head)
    assert head["reachable"] == lattice["reachable"] == stats["tsdf_path_reachable"]
    assert head["lattice_length_m"] == lattice["length_m"] and head["n_lattice_points"] == lattice["n_points"]
    assert stats["tsdf_path_straight_length_m"] == head["length_m"] and stats["tsdf_path_waypoints"] == head["n_points"]
    assert head["n_points"] == len(points)
    if head["reachable"]:
        assert 1 <= head["n_points"] <= lattice["n_points"] and head["length_m"] <= lattice["length_m"]
        assert head["min_clearance_m"] > 0.2
        assert np.array_equal(points[0], lattice_points[0]) and np.array_equal(points[-1], lattice_points[-1])
        legs = np.linalg.norm(np.diff(points, axis=0), axis=1).sum()
        assert abs(legs - head["length_m"]) < 1e-4 * max(1, len(points))      # a leg is rounded down to a milli-voxel
    else:
        assert head["n_points"] == 0 and head["length_m"] == math.inf
    EG.TG.whole_run(without_dir, cfg(plan_cfg))
    assert "tsdf_path_straight_length_m" not in returned[1] and "tsdf_path_waypoints" not in returned[1]
    assert returned[1]["tsdf_path_length_m"] == stats["tsdf_path_length_m"]
    straight = os.path.join("map", "path_straight.txt")
    listed = EG.TG.listing(with_dir)
    assert straight in listed and [p for p in listed if p != straight] == EG.TG.listing(without_dir)
    assert open(f"{with_dir}/map/path.txt").read() == open(f"{without_dir}/map/path.txt").read()
