"""The cost-to-go field and its paths on the MI355X (csrc/geodesic.hip, go_slam_amd/plan.py, ESDF.plan): the field and
the walked cells equal the serial restatement (tests/geodesic_restatement.py) with torch.equal -- on a random lattice with
a ragged tail and bricks cut on every axis, on a serpentine that needs many sweeps, at the smallest sizes, with several
seeds and on the hand cases of the corner rule; a hand-built room with a door is planned through end to end; and an
only-tracking run with tsdf.esdf.plan ends with map/path.txt."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import geodesic_restatement as GR                              # noqa: E402
import test_esdf_gpu as EG                                     # noqa: E402  (its only-tracking run)
import test_geodesic_cpu as GC                                 # noqa: E402  (the hand cases)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INF = GR.INF
_REF = {}


def random_lattice():
    passable = np.random.default_rng(0).random((9, 11, 70)) > 0.35
    passable[4, 5, 3] = True
    return passable


def serpentine():
    """3 x 17 x 70: every odd row of axis 1 is a wall with a two-cell gap, at alternating ends of axis 2."""
    passable = np.ones((3, 17, 70), dtype=bool)
    for n, j in enumerate(range(1, 17, 2)):
        passable[:, j, :] = False
        if n % 2 == 0:
            passable[:, j, 68:] = True
        else:
            passable[:, j, :2] = True
    return passable


def reference(name, passable, seeds, max_cost=GR.MAX_COST):
    """The restatement's field, computed once per named case and left unchanged."""
    key = (name, max_cost)
    if key not in _REF:
        _REF[key] = GR.field(passable, seeds, max_cost)
        _REF[key].setflags(write=False)
    return _REF[key]


def gpu_field(passable, seeds, max_cost=None, **kw):
    from go_slam_amd import plan
    return plan.geodesic_field(torch.from_numpy(np.ascontiguousarray(passable)).to(DEV), seeds, max_cost, **kw)


def assert_field(field, ref):
    assert field.cost.dtype == torch.int32 and field.dims == ref.shape and field.sweeps >= 1
    assert torch.equal(field.cost.cpu(), torch.from_numpy(np.array(ref)))


@pytest.mark.parametrize("max_cost", [None, 20000])
def test_random_lattice_equals_the_restatement(built_lib, max_cost):
    passable = random_lattice()
    ref = reference("random", passable, [(4, 5, 3)], GR.MAX_COST if max_cost is None else max_cost)
    reached = int((ref < INF).sum())
    print("reached", reached, "of", ref.size)
    assert reached >= ref.size // 2 if max_cost is None else reached == 1206        # not vacuous
    field = gpu_field(passable, [(4, 5, 3)], max_cost)
    print("sweeps", field.sweeps)
    assert_field(field, ref)


def test_serpentine_needs_many_sweeps_and_max_sweeps_is_an_orderly_error(built_lib):
    from go_slam_amd import plan
    passable = serpentine()
    ref = reference("serpentine", passable, [(1, 0, 0)])
    assert (ref < INF).sum() == passable.sum() and ref.max() > 9 * 66 * 1000
    field = gpu_field(passable, [(1, 0, 0)])
    print("sweeps", field.sweeps, "brick", plan.brick())
    assert_field(field, ref)
    # a brick sees what its neighbour lowered only in the next sweep, so each of the nine corridors costs a sweep per
    # brick boundary it crosses along axis 2: only bricks re-marked by their neighbours' flags get that far
    crossings = 9 * ((70 + plan.brick()[2] - 1) // plan.brick()[2] - 1)
    assert crossings < field.sweeps <= 65536
    with pytest.raises(RuntimeError, match="max_sweeps"):
        gpu_field(passable, [(1, 0, 0)], max_sweeps=1)
    torch.cuda.synchronize()
    assert_field(gpu_field(passable, [(1, 0, 0)], max_sweeps=field.sweeps + 64), ref)     # the device is fine afterwards


@pytest.mark.parametrize("dims", [(1, 1, 1), (1, 5, 7), (2, 2, 2)], ids=lambda d: "x".join(map(str, d)))
def test_smallest_lattices(built_lib, dims):
    passable = np.random.default_rng(sum(dims)).random(dims) > 0.25
    passable[0, 0, 0] = True
    assert_field(gpu_field(passable, [(0, 0, 0)]), GR.field(passable, [(0, 0, 0)]))
    assert_field(gpu_field(passable, [(0, 0, 0)], 1500), GR.field(passable, [(0, 0, 0)], 1500))
    full = np.ones(dims, dtype=bool)
    last = tuple(n - 1 for n in dims)
    assert_field(gpu_field(full, [last]), GR.field(full, [last]))


def test_several_seeds_a_duplicate_and_seeds_on_faces(built_lib):
    passable = random_lattice()
    seeds = [(0, 0, 0), (8, 10, 69), (4, 5, 3), (4, 5, 3), (0, 10, 35), (8, 0, 64), (3, 7, 16)]
    for s in seeds:
        passable[s] = True
    passable[3, 7, 16] = False                              # a blocked seed among them is ignored
    ref = GR.field(passable, seeds)
    assert all(ref[s] == 0 for s in seeds[:-1]) and ref[3, 7, 16] == INF
    assert_field(gpu_field(passable, np.array(seeds)), ref)
    assert_field(gpu_field(passable, torch.tensor(seeds, dtype=torch.int32, device=DEV)), ref)


@pytest.mark.parametrize("case", GC.corner_cases(), ids=lambda c: c[0])
def test_hand_cases_of_the_corner_rule(built_lib, case):
    _, passable, seeds, max_cost, want = case
    field = gpu_field(passable, seeds, max_cost)
    assert torch.equal(field.cost.cpu(), torch.from_numpy(want))


@pytest.mark.parametrize("name", ["random", "serpentine"])
def test_path_equals_the_restatement(built_lib, name):
    passable, seed = (random_lattice(), (4, 5, 3)) if name == "random" else (serpentine(), (1, 0, 0))
    ref = reference(name, passable, [seed])
    field = gpu_field(passable, [seed])
    far = np.unravel_index(np.argmax(np.where(ref < INF, ref, -1)), ref.shape)
    mid = tuple(np.argwhere((ref < INF) & (ref > ref[far] // 2))[0])
    for start in (far, mid, seed):
        want, n = GR.path(ref, passable, start, ref.size)
        got = field.path(start)
        assert got.dtype == torch.int32 and n == len(want) >= 1
        assert torch.equal(got.cpu(), torch.from_numpy(want))
        GC.check_path(ref, passable, got.cpu().numpy(), start)
        assert torch.equal(field.path(np.array(start), max_len=n).cpu(), torch.from_numpy(want))
    print(name, "longest path", len(GR.path(ref, passable, far, ref.size)[0]), "cells, cost", ref[far])
    unreachable = np.argwhere(ref >= INF)
    if len(unreachable):
        assert tuple(field.path(unreachable[0]).shape) == (0, 3)
    with pytest.raises(ValueError, match="outside the lattice"):
        field.path((0, 0, ref.shape[2]))
    with pytest.raises(ValueError, match="max_len"):
        field.path(seed, max_len=0)


def test_c_abi_short_max_len_and_bad_arguments(built_lib):
    from go_slam_amd import _lib
    L = _lib.lib()
    passable = random_lattice()
    ref = reference("random", passable, [(4, 5, 3)])
    field = gpu_field(passable, [(4, 5, 3)])
    far = [int(v) for v in np.unravel_index(np.argmax(np.where(ref < INF, ref, -1)), ref.shape)]
    n_true = GR.path(ref, passable, far, ref.size)[1]
    assert n_true > 2
    cells = torch.full((n_true, 3), -7, dtype=torch.int32, device=DEV)
    n = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    stream = _lib.stream_ptr(DEV)
    P = _lib.ptr
    dims = (9, 11, 70)

    def walk(start, max_len):
        rc = L.gs_geodesic_path(P(field.cost), P(field.passable), *dims, *start, max_len, P(cells), P(n), stream)
        assert rc == 0
        return int(n.item())
    assert walk(far, n_true - 1) == -1
    assert (cells[n_true - 1] == -7).all()                  # nothing past max_len was written
    assert walk(far, n_true) == n_true
    assert walk([9, 0, 0], 2) == 0 and walk([0, -1, 0], 2) == 0
    assert walk([int(v) for v in np.argwhere(ref >= INF)[0]], 2) == 0

    INVALID = -1
    cost, flags = field.cost, torch.zeros(L.gs_geodesic_flags_bytes(*dims), dtype=torch.uint8, device=DEV)
    before = cost.clone()
    changed = torch.zeros(8, dtype=torch.int32, device=DEV)
    seeds = torch.tensor([[4, 5, 3]], dtype=torch.int32, device=DEV)
    assert L.gs_geodesic_flags_bytes(0, 1, 1) == 0 and L.gs_geodesic_flags_bytes(1, 1025, 1) == 0
    from go_slam_amd import plan
    b0, b1, b2 = plan.brick()
    assert L.gs_geodesic_flags_bytes(*dims) == 2 * -(-9 // b0) * -(-11 // b1) * -(-70 // b2)
    for bad in ((0, 11, 70), (9, 1025, 70), (9, 11, -1)):
        assert L.gs_geodesic_init(P(field.passable), *bad, P(seeds), 1, P(cost), P(flags), stream) == INVALID
        assert L.gs_geodesic_relax(P(field.passable), *bad, 5, P(cost), P(flags), 0, 1, P(changed), stream) == INVALID
        assert L.gs_geodesic_path(P(cost), P(field.passable), *bad, 0, 0, 0, 4, P(cells), P(n), stream) == INVALID
    assert L.gs_geodesic_init(P(field.passable), *dims, P(seeds), -1, P(cost), P(flags), stream) == INVALID
    assert L.gs_geodesic_init(P(field.passable), *dims, None, 1, P(cost), P(flags), stream) == INVALID
    assert L.gs_geodesic_init(None, *dims, P(seeds), 1, P(cost), P(flags), stream) == INVALID
    assert L.gs_geodesic_init(P(field.passable), *dims, P(seeds), 1, None, P(flags), stream) == INVALID
    assert L.gs_geodesic_init(P(field.passable), *dims, P(seeds), 1, P(cost), None, stream) == INVALID
    for max_cost in (-1, GR.MAX_COST + 1):
        assert L.gs_geodesic_relax(P(field.passable), *dims, max_cost, P(cost), P(flags), 0, 1, P(changed),
                                   stream) == INVALID
    for sweep0, k in ((0, 0), (-1, 1), (0, -2)):
        assert L.gs_geodesic_relax(P(field.passable), *dims, 5, P(cost), P(flags), sweep0, k, P(changed),
                                   stream) == INVALID
    assert L.gs_geodesic_relax(P(field.passable), *dims, 5, P(cost), P(flags), 0, 1, None, stream) == INVALID
    assert L.gs_geodesic_path(P(cost), P(field.passable), *dims, 0, 0, 0, 0, P(cells), P(n), stream) == INVALID
    assert L.gs_geodesic_path(P(cost), P(field.passable), *dims, 0, 0, 0, 4, P(cells), None, stream) == INVALID
    assert L.gs_geodesic_brick(None, None, None) == INVALID
    assert b"geodesic" in L.gs_last_error()
    torch.cuda.synchronize()
    assert torch.equal(cost, before)                        # nothing was launched


# ---- end to end on a hand-built volume ------------------------------------------------------------------------------
VOXEL = 0.125
ROOM = (40, 24, 40)
WALL_X = (19, 20)                                           # the wall's two layers
DOOR_Y, DOOR_Z = (1, 14), (16, 23)                          # the opening, inclusive


@pytest.fixture(scope="module")
def room(built_lib):
    """A box room, solid shell, split by a wall with one door, written straight into a TSDFVolume; its distance field."""
    from go_slam_amd.tsdf import TSDFVolume
    bound = [[0.0, (n - 1) * VOXEL] for n in ROOM]
    vol = TSDFVolume(bound, VOXEL, device=DEV)
    assert vol.dims == ROOM
    t = np.ones(ROOM, dtype=np.float32)
    t[0], t[-1], t[:, 0], t[:, -1], t[:, :, 0], t[:, :, -1] = -1, -1, -1, -1, -1, -1
    t[WALL_X[0]:WALL_X[1] + 1] = -1
    t[WALL_X[0]:WALL_X[1] + 1, DOOR_Y[0]:DOOR_Y[1] + 1, DOOR_Z[0]:DOOR_Z[1] + 1] = 1
    vol.tsdf.copy_(torch.from_numpy(t))
    vol.weight.fill_(1.0)
    vol._flags = None
    return vol, vol.esdf()


START, GOAL = (8 * VOXEL, 6 * VOXEL, 30 * VOXEL), (33 * VOXEL, 16 * VOXEL, 6 * VOXEL)


def in_door(cells):
    c = np.asarray(cells)
    return ((c[:, 0] >= WALL_X[0]) & (c[:, 0] <= WALL_X[1]) & (c[:, 1] >= DOOR_Y[0]) & (c[:, 1] <= DOOR_Y[1])
            & (c[:, 2] >= DOOR_Z[0]) & (c[:, 2] <= DOOR_Z[1]))


def test_plan_goes_through_the_door_and_equals_the_restatement(room):
    from go_slam_amd import plan
    vol, field = room
    radius = VOXEL
    res = field.plan(START, GOAL, robot_radius=radius)
    passable = field.passable(radius)
    p = passable.cpu().numpy() != 0
    assert res["reachable"] and res["start_cell"] == [8, 6, 30] and res["goal_cell"] == [33, 16, 6]
    cells = res["cells"].cpu().numpy()
    assert in_door(cells).sum() >= 2 and p[tuple(cells.T)].all()
    assert (cells[in_door(cells)][:, 2] >= 18).all() and (cells[in_door(cells)][:, 2] <= 21).all()   # a voxel off the jambs
    print("length_m", res["length_m"], "min_clearance_m", res["min_clearance_m"], "sweeps", res["sweeps"], len(cells))
    assert res["min_clearance_m"] >= radius
    assert res["min_clearance_m"] == float(field.dist.cpu().numpy()[tuple(cells.T)].min())
    ref = GR.field(p, [res["goal_cell"]])
    g = plan.geodesic_field(passable, [res["goal_cell"]])
    assert torch.equal(g.cost.cpu(), torch.from_numpy(ref))
    want, n = GR.path(ref, p, res["start_cell"], ref.size)
    assert n == len(cells) and np.array_equal(cells, want)
    assert res["length_m"] == float(ref[8, 6, 30]) * VOXEL / 1000.0
    straight = math.dist(START, GOAL)
    assert straight < res["length_m"] < 2.0 * straight
    assert res["points"].dtype == torch.float64
    assert np.array_equal(res["points"].cpu().numpy(), cells.astype(np.float64) * VOXEL)          # lo = 0
    # a cap below the route's length makes it unreachable, one above leaves it alone
    assert not field.plan(START, GOAL, robot_radius=radius, max_cost_m=res["length_m"] - 0.01)["reachable"]
    again = field.plan(START, GOAL, robot_radius=radius, max_cost_m=res["length_m"] + 0.01)
    assert again["reachable"] and torch.equal(again["cells"], res["cells"])


def test_a_robot_wider_than_the_door_stays_on_its_side(room):
    vol, field = room
    wide = 4 * VOXEL                                        # the door is 8 cells wide: no cell of it is > 4 voxels from a jamb
    res = field.plan(START, GOAL, robot_radius=wide)
    assert res["reachable"] is False and res["cells"].shape[0] == 0 and res["length_m"] == math.inf
    assert math.isnan(res["min_clearance_m"]) and res["sweeps"] >= 1
    reach = field.reachable([START], robot_radius=wide)
    assert reach.dtype == torch.bool and tuple(reach.shape) == ROOM
    free = field.state == 1
    assert reach[8, 6, 30] and reach[:WALL_X[0]].sum() > 1000
    assert not reach[WALL_X[1] + 1:].any() and free[WALL_X[1] + 1:].sum() > 1000
    both = field.reachable([START, GOAL], robot_radius=wide)
    assert both[33, 16, 6] and both[8, 6, 30]
    slim = field.reachable(torch.tensor([START]), robot_radius=VOXEL)
    assert slim[33, 16, 6] and torch.equal(slim, field.passable(VOXEL) != 0)      # one connected free space


def test_snap_moves_an_endpoint_out_of_the_wall(room):
    vol, field = room
    inside_wall = (19 * VOXEL, 6 * VOXEL, 5 * VOXEL)
    assert field.plan(inside_wall, GOAL, robot_radius=VOXEL)["start_cell"] is None
    res = field.plan(inside_wall, GOAL, robot_radius=VOXEL, snap=3 * VOXEL)
    # passable needs d2 > 1: x = 18 is a site, x = 17 one voxel from it, so x = 16 is the nearest passable layer, three
    # cells from the wall's layer x = 19 (the far side's, x = 23, is four away)
    assert res["start_cell"] == [16, 6, 5] and res["reachable"]
    assert field.plan(inside_wall, GOAL, robot_radius=VOXEL, snap=2.9 * VOXEL)["start_cell"] is None
    outside = (-2 * VOXEL, 6 * VOXEL, 5 * VOXEL)            # the shell x = 0, the site x = 1, then x = 3 is passable
    assert field.plan(outside, GOAL, robot_radius=VOXEL, snap=5 * VOXEL)["start_cell"] == [3, 6, 5]


def test_plan_on_map_finds_the_door(room):
    from go_slam_amd import plan
    vol, field = room
    grid = field.occupancy_slice(1, (6 * VOXEL, 8 * VOXEL), robot_radius=VOXEL)
    res = plan.plan_on_map(grid, (START[0], START[2]), (GOAL[0], GOAL[2]))
    assert res["reachable"] and res["start_cell"] == (8, 30) and res["goal_cell"] == (33, 6)
    cells = res["cells"].cpu().numpy()
    through = cells[(cells[:, 0] >= WALL_X[0]) & (cells[:, 0] <= WALL_X[1])]
    assert len(through) >= 2 and (through[:, 1] >= DOOR_Z[0]).all() and (through[:, 1] <= DOOR_Z[1]).all()
    free = grid["cells"].cpu().numpy() == 254
    ref = GR.field(free[None], [(0, 33, 6)])
    want, n = GR.path(ref, free[None], (0, 8, 30), ref.size)
    assert n == len(cells) and np.array_equal(cells, want[:, 1:])
    assert res["length_m"] == float(ref[0, 8, 30]) * VOXEL / 1000.0
    centres = np.array(grid["origin"]) + (cells.astype(np.float64) + 0.5) * VOXEL
    assert np.array_equal(res["points"].cpu().numpy(), centres)
    grid_wide = field.occupancy_slice(1, (6 * VOXEL, 8 * VOXEL), robot_radius=4 * VOXEL)
    assert not plan.plan_on_map(grid_wide, (START[0], START[2]), (GOAL[0], GOAL[2]))["reachable"]


# ---- whole run ------------------------------------------------------------------------------------------------------
def test_only_tracking_run_ends_with_a_path_file(built_lib, tmp_path, monkeypatch):
    from go_slam_amd import plan
    from go_slam_amd.slam import SLAM
    returned = []
    terminate = SLAM.terminate

    def keeping(self, *args, **kw):
        returned.append(terminate(self, *args, **kw))
        return returned[-1]
    monkeypatch.setattr(SLAM, "terminate", keeping)
    esdf_cfg = {"enable": True, "max_distance": 1.0,
                "slice": {"up_axis": 1, "height": [-0.5, 0.5], "robot_radius": 0.2}}
    with_dir, without_dir = str(tmp_path / "with"), str(tmp_path / "without")
    EG.TG.whole_run(with_dir, {"enable": True, "source": "sensor", "voxel_size": 0.1,
                               "esdf": {**esdf_cfg, "plan": {"enable": True, "robot_radius": 0.2, "snap": 1.0,
                                                          "allow_unknown": True, "goal": [0.6, 0.0, 0.3]}}})
    stats = returned[0]
    head, points = plan.parse_path(open(f"{with_dir}/map/path.txt").read())
    print("map/path.txt:", head)
    assert stats["tsdf_path_reachable"] == head["reachable"]
    assert stats["tsdf_path_length_m"] == head["length_m"] and head["n_points"] == len(points)
    if head["reachable"]:
        assert head["n_points"] >= 1 and head["min_clearance_m"] >= 0.2 and math.isfinite(head["length_m"])
        steps = np.linalg.norm(np.diff(points, axis=0), axis=1)
        assert (steps < 0.1 * 1.7321 + 1e-9).all() and abs(steps.sum() - head["length_m"]) < 1e-3 * max(1, len(steps))
    else:
        assert head["n_points"] == 0 and head["length_m"] == math.inf
    EG.TG.whole_run(without_dir, {"enable": True, "source": "sensor", "voxel_size": 0.1, "esdf": esdf_cfg})
    assert "tsdf_path_reachable" not in returned[1] and "tsdf_path_length_m" not in returned[1]
    listed = EG.TG.listing(with_dir)
    assert os.path.join("map", "path.txt") in listed
    assert [p for p in listed if p != os.path.join("map", "path.txt")] == EG.TG.listing(without_dir)
