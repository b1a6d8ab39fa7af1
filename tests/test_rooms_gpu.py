"""csrc/rooms.hip on the device against tests/rooms_restatement.py, output by output and exactly: on the hand plan, flat
and replicated into sheets, on a random lattice with a ragged tail, on a serpentine whose labels cross many bricks, at the
smallest sizes, without any core, through the corner where eight bricks meet, with a dropped core, with and without d2;
the C ABI's refusals; then `ESDF.rooms` on a hand-built two-room volume and a whole run that ends with map/rooms.txt."""
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import geodesic_restatement as GR                              # noqa: E402
import rooms_restatement as RR                                 # noqa: E402
import test_esdf_gpu as EG                                     # noqa: E402  (its only-tracking run)
import test_geodesic_gpu as GG                                 # noqa: E402  (its serpentine and its room)
import test_rooms_cpu as RC                                    # noqa: E402  (the lattices and their references)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INF = GR.INF
reference = RC.reference


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def gpu_segments(open_, core, d2=None, **kw):
    from go_slam_amd import rooms
    return rooms.room_segments(dev(open_), dev(core), dev(d2), **kw)


def assert_segments(seg, ref):
    """Every output equals the restatement's."""
    from go_slam_amd import rooms
    for name in ("label", "cost", "door_label"):
        got = getattr(seg, name)
        assert got.dtype == torch.int32 and tuple(got.shape) == ref[name].shape
        assert np.array_equal(got.cpu().numpy(), ref[name]), name
    assert seg.counts.cpu().tolist() == ref["counts"].tolist()
    assert seg.n_rooms == len(ref["rooms"]["root"]) and seg.n_doors == len(ref["doors"]["root"])
    for table, want, columns in ((seg.rooms, ref["rooms"], rooms.ROOM_COLUMNS),
                                 (seg.doors, ref["doors"], rooms.DOOR_COLUMNS)):
        for c in columns:
            got = table[c].cpu().numpy()
            assert got.dtype == want[c].dtype and got.shape == want[c].shape, (c, got.dtype, got.shape)
            assert np.array_equal(got, want[c]), c
    assert np.array_equal(seg.core_roots.cpu().numpy(), ref["core_roots"])
    assert np.array_equal(seg.core_sizes.cpu().numpy(), ref["core_sizes"])
    row = {int(r): i for i, r in enumerate(ref["rooms"]["root"])}
    want_room = np.vectorize(lambda v: row.get(int(v), -1), otypes=[np.int32])(ref["label"])
    assert np.array_equal(seg.room.cpu().numpy(), want_room)
    assert seg.doors["room_a"].cpu().tolist() == [row[int(v)] for v in ref["doors"]["room_lo"]]
    assert seg.doors["room_b"].cpu().tolist() == [row[int(v)] for v in ref["doors"]["room_hi"]]
    assert set(seg.sweeps) == {"cores", "cost", "rooms", "doors"} and all(v >= 1 for v in seg.sweeps.values())


def cells_with_parents_of_two_labels(open_, ref):
    ok = GR.move_masks(open_)
    n = 0
    for c in np.argwhere((ref["label"] >= 0) & (ref["cost"] > 0)):
        c = tuple(int(v) for v in c)
        seen = set()
        for m, (d, w) in enumerate(zip(GR.MOVES, GR.WEIGHTS)):
            q = (c[0] + d[0], c[1] + d[1], c[2] + d[2])
            if ok[(m,) + c] and int(ref["cost"][q]) + w == int(ref["cost"][c]):
                seen.add(int(ref["label"][q]))
        n += len(seen) > 1
    return n


# ---- the lattices -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_d2", [True, False])
def test_hand_plan_equals_the_restatement(built_lib, with_d2):
    open_, core, d2 = RC.hand_plan()
    ref = reference("hand", open_, core, d2 if with_d2 else None)
    assert ref["rooms"]["size"].tolist() == [789, 403, 330] and ref["doors"]["size"].tolist() == [10, 8]
    seg = gpu_segments(open_, core, d2 if with_d2 else None)
    print("sweeps", seg.sweeps)
    assert_segments(seg, ref)
    graph = seg.graph()
    assert graph["doors"] == [(0, 1), (1, 2)]
    assert graph["rooms"] == [{"doors": [0], "neighbours": [1]}, {"doors": [0, 1], "neighbours": [0, 2]},
                              {"doors": [1], "neighbours": [1]}]
    assert seg.room_at((0, 10, 10)) == 0 and seg.room_at((0, 10, 50)) == 1 and seg.room_at((0, 30, 50)) == 2
    assert seg.room_at((0, 0, 0)) == -1
    # a hand-made walk from the left room through both openings
    walk = [(0, 10, z) for z in range(10, 48)] + [(0, y, 47) for y in range(11, 31)]
    along = seg.rooms_along(torch.tensor(walk))
    assert along["rooms"] == [0, 1, 2] and sum(along["cells"]) == len(walk) and along["doors"] == [0, 1]
    assert seg.rooms_along(torch.zeros((0, 3), dtype=torch.int32)) == {"rooms": [], "cells": [], "doors": []}


def test_other_radii_and_a_larger_least_core(built_lib):
    open4, core4, _ = RC.hand_plan(1, 4)
    merged = reference("hand 1 4", open4, core4)
    assert len(merged["rooms"]["root"]) == 2 and len(merged["doors"]["root"]) == 1
    assert_segments(gpu_segments(open4, core4), merged)
    open_, core, d2 = RC.hand_plan()
    one = reference("hand", open_, core, d2, min_core_cells=200)
    assert len(one["rooms"]["root"]) == 1 and len(one["doors"]["root"]) == 0
    assert_segments(gpu_segments(open_, core, d2, min_core_cells=200), one)


def test_hand_plan_in_sheets_equals_the_restatement(built_lib):
    """[6,40,64]: bricks are cut on every axis and the doorways are sheets."""
    open_, core, d2 = (np.repeat(a, 6, axis=0) for a in RC.hand_plan())
    ref = reference("hand sheets", open_, core, d2)
    assert len(ref["rooms"]["root"]) == 3 and ref["doors"]["size"].tolist() == [60, 48]
    assert_segments(gpu_segments(open_, core, d2), ref)


def test_random_lattice_equals_the_restatement(built_lib):
    open_, core, d2 = RC.random_lattice()
    ref = reference("random", open_, core, d2)
    ties = cells_with_parents_of_two_labels(open_, ref)
    print("rooms", len(ref["rooms"]["root"]), "doors", len(ref["doors"]["root"]), "cells with parents of two labels", ties)
    assert len(ref["rooms"]["root"]) >= 8 and len(ref["doors"]["root"]) >= 1 and ties >= 1       # not vacuous
    seg = gpu_segments(open_, core, d2)
    print("sweeps", seg.sweeps)
    assert_segments(seg, ref)
    capped = reference("random", open_, core, d2, max_cost=3000)
    assert (capped["label"] >= 0).sum() < (ref["label"] >= 0).sum()
    assert_segments(gpu_segments(open_, core, d2, max_cost=3000), capped)


def test_serpentine_needs_more_than_one_sweep_and_max_sweeps_is_an_orderly_error(built_lib):
    open_ = GG.serpentine()
    core = np.zeros_like(open_)
    # the first cell of the nine corridors and the last but one: the route between them has an odd number of cells, so
    # its middle cell is as far from one core as from the other
    core[1, 0, 0] = core[1, 16, 68] = True
    ref = reference("serpentine", open_, core)
    assert len(ref["rooms"]["root"]) == 2 and (ref["label"] >= 0).sum() == open_.sum()
    assert len(ref["doors"]["root"]) == 1 and cells_with_parents_of_two_labels(open_, ref) >= 1
    assert ref["cost"][1, 8, 34] == ref["cost"][1, 8, 35] + 1000 and ref["label"][1, 8, 34] == ref["rooms"]["root"][0]
    assert ref["label"][1, 8, 35] == ref["rooms"]["root"][1]                  # the tie went to the lower root
    seg = gpu_segments(open_, core)
    print("sweeps", seg.sweeps)
    assert_segments(seg, ref)
    assert seg.sweeps["rooms"] > 1 and seg.sweeps["cost"] > 1
    with pytest.raises(RuntimeError, match="max_sweeps"):
        gpu_segments(open_, core, max_sweeps=1)
    torch.cuda.synchronize()
    assert_segments(gpu_segments(open_, core), ref)         # the device is fine afterwards


@pytest.mark.parametrize("dims", [(1, 1, 1), (1, 5, 7), (2, 2, 2)], ids=lambda d: "x".join(map(str, d)))
def test_smallest_lattices(built_lib, dims):
    rng = np.random.default_rng(sum(dims))
    open_ = rng.random(dims) < 0.8
    open_[0, 0, 0] = True
    core = np.zeros(dims, dtype=bool)
    core[0, 0, 0] = core[-1, -1, -1] = True
    core &= open_
    d2 = rng.integers(0, 9, dims).astype(np.int32)
    assert_segments(gpu_segments(open_, core, d2), RR.segments(open_, core, d2))


def test_no_core_at_all(built_lib):
    open_, _, d2 = RC.random_lattice()
    core = np.zeros_like(open_)
    seg = gpu_segments(open_, core, d2)
    assert seg.n_rooms == 0 and seg.n_doors == 0 and (seg.label == -1).all() and (seg.room == -1).all()
    assert (seg.cost == INF).all() and (seg.door_label == -1).all()
    assert seg.rooms["sum"].shape == (0, 3) and seg.rooms["bbox"].shape == (0, 6) and seg.doors["bbox"].shape == (0, 6)
    assert seg.graph() == {"doors": [], "rooms": []}
    assert_segments(seg, RR.segments(open_, core, d2))


def test_two_rooms_that_meet_only_through_the_corner_where_eight_bricks_join(built_lib):
    from go_slam_amd import frontier
    b = frontier.brick()
    dims = tuple(n + 1 for n in b)                          # one brick plus one cell on every axis: 5 x 5 x 33
    a = tuple(n - 1 for n in b)                             # the last cell of brick (0,0,0)
    open_ = np.zeros(dims, dtype=bool)
    open_[a[0]:, a[1]:, a[2]:] = True                       # the 2 x 2 x 2 box around the corner: a cell of every brick
    open_[a[0], a[1], a[2] - 3:] = True                     # a corridor inside brick (0,0,0)
    core = np.zeros(dims, dtype=bool)
    core[a[0], a[1], a[2] - 3] = core[b] = True             # its far end, and the only cell of brick (1,1,1)
    ref = RR.segments(open_, core)
    far = int(np.ravel_multi_index(b, dims))
    assert ref["rooms"]["root"].tolist() == [int(np.ravel_multi_index((a[0], a[1], a[2] - 3), dims)), far]
    assert ref["label"][a] == far and ref["cost"][a] == 1732               # the diagonal through the corner
    assert (ref["label"][a[0]:, a[1]:, a[2]:] == far).all() and len(ref["doors"]["root"]) == 1
    assert_segments(gpu_segments(open_, core), ref)


def test_min_core_cells_drops_a_core_between_two_kept_ones(built_lib):
    open_, core = RC.corridor()
    plain = reference("corridor", open_, core)
    core = core.copy()
    core[0, 1, 20] = True                                   # one cell, in the middle
    ref = RR.segments(open_, core, None, 2)
    assert ref["core_sizes"].tolist() == [3, 3, 1] and ref["rooms"]["root"].tolist() == [0, 40]
    assert np.array_equal(ref["label"], plain["label"]) and ref["label"][0, 1, 20] == 0      # the tie, at a dropped core
    assert_segments(gpu_segments(open_, core, min_core_cells=2), ref)
    three = RR.segments(open_, core)
    assert len(three["rooms"]["root"]) == 3 and len(three["doors"]["root"]) == 2
    assert_segments(gpu_segments(open_, core), three)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------
def test_c_abi_refuses_bad_arguments_and_writes_nothing(built_lib):
    from go_slam_amd import _lib
    L = _lib.lib()
    P = _lib.ptr
    stream = _lib.stream_ptr(DEV)
    INVALID = -1
    open_h, core_h, d2_h = RC.random_lattice()
    dims = open_h.shape
    n = open_h.size
    open_, core, d2 = dev(open_h.astype(np.uint8)), dev(core_h.astype(np.uint8)), dev(d2_h)

    def filled(count, dtype):
        return torch.full((count,), 113, dtype=dtype, device=DEV)
    label, door, cost = filled(n, torch.int32), filled(n, torch.int32), filled(n, torch.int32)
    counts, changed = filled(4, torch.int32), filled(8, torch.int32)
    flags = filled(L.gs_frontier_flags_bytes(*dims), torch.uint8)
    ws_bytes = L.gs_frontier_workspace_bytes(*dims)
    ws = filled(ws_bytes, torch.uint8)
    K = 4
    i32 = {k: filled(6 * K, torch.int32) for k in ("root", "size", "core_size", "bbox", "reach", "lo", "hi")}
    keep = filled(K, torch.uint8)
    total, widest = filled(3 * K, torch.int64), filled(K, torch.int64)
    everything = [label, door, cost, counts, changed, flags, ws, keep, total, widest] + list(i32.values())

    def calls(only, d=dims, drop=None, rows=K, capacity=K, wb=ws_bytes):
        """The entries `only` once each, every one with a bad argument; `drop` names the argument passed as NULL."""
        def a(name, t):
            return None if name == drop else P(t)
        entries = {
            "mark": lambda: L.gs_room_mark(a("open", open_), a("core", core), *d, a("label", label), a("counts", counts),
                                   a("flags", flags), stream),
            "cores": lambda: L.gs_room_cores(a("label", label), *d, a("ws", ws), wb, rows, capacity, a("root", i32["root"]),
                                     P(i32["size"]), stream),
            "seed": lambda: L.gs_room_seed(a("open", open_), *d, a("root", i32["root"]), a("keep", keep), rows, a("label", label),
                                   a("flags", flags), stream),
            "relax": lambda: L.gs_room_relax(a("open", open_), a("cost", cost), *d, a("label", label), a("flags", flags), 0, 1,
                                     a("changed", changed), stream),
            "door_mark": lambda: L.gs_room_door_mark(a("open", open_), a("label", label), *d, a("door", door), a("counts", counts),
                                             a("flags", flags), stream),
            "table": lambda: L.gs_room_table(a("label", label), a("cost", cost), *d, a("root", i32["root"]), rows, a("size", i32["size"]),
                                     a("core_size", i32["core_size"]), a("total", total), a("bbox", i32["bbox"]),
                                     a("reach", i32["reach"]), stream),
            "door_table": lambda: L.gs_room_door_table(a("open", open_), a("label", label), a("door", door), P(d2), *d,
                                               a("root", i32["root"]), rows, a("size", i32["size"]), a("total", total),
                                               a("bbox", i32["bbox"]), a("lo", i32["lo"]), a("hi", i32["hi"]),
                                               a("widest", widest), stream)}
        return {e: entries[e]() for e in only}

    uses = {"open": ("mark", "seed", "relax", "door_mark", "door_table"), "core": ("mark",), "counts": ("mark", "door_mark"),
            "label": ("mark", "cores", "seed", "relax", "door_mark", "table", "door_table"), "ws": ("cores",),
            "flags": ("mark", "seed", "relax", "door_mark"), "root": ("cores", "seed", "table", "door_table"),
            "keep": ("seed",), "cost": ("relax", "table"), "changed": ("relax",), "door": ("door_mark", "door_table"),
            "size": ("table", "door_table"), "core_size": ("table",), "bbox": ("table", "door_table"), "reach": ("table",),
            "total": ("table", "door_table"), "lo": ("door_table",), "hi": ("door_table",), "widest": ("door_table",)}
    every = ("mark", "cores", "seed", "relax", "door_mark", "table", "door_table")
    for bad in ((0, 13, 70), (9, 1025, 70), (9, 13, -1)):
        assert set(calls(every, d=bad).values()) == {INVALID}, bad
    for name, entries in uses.items():
        assert set(calls(entries, drop=name).values()) == {INVALID}, name
    assert set(calls(("cores", "seed", "table", "door_table"), rows=-1).values()) == {INVALID}
    assert calls(("cores",), capacity=K - 1)["cores"] == INVALID and calls(("cores",), wb=ws_bytes - 1)["cores"] == INVALID
    for sweep in ((0, 0), (-1, 1), (0, -2), (0x7fffffff, 1)):
        assert L.gs_room_relax(P(open_), P(cost), *dims, P(label), P(flags), sweep[0], sweep[1], P(changed),
                               stream) == INVALID
    # a 64-bit column four bytes off
    assert L.gs_room_table(P(label), P(cost), *dims, P(i32["root"]), K, P(i32["size"]), P(i32["core_size"]),
                           P(total.view(torch.int32)[1:]), P(i32["bbox"]), P(i32["reach"]), stream) == INVALID
    assert L.gs_room_door_table(P(open_), P(label), P(door), None, *dims, P(i32["root"]), K, P(i32["size"]), P(total),
                                P(i32["bbox"]), P(i32["lo"]), P(i32["hi"]), P(widest.view(torch.int32)[1:]),
                                stream) == INVALID
    assert b"room" in L.gs_last_error()
    torch.cuda.synchronize()
    for t in everything:
        assert (t == 113).all()                             # nothing was launched, nothing was cleared
    # no rows: nothing to do, nothing written
    assert L.gs_room_cores(P(label), *dims, P(ws), ws_bytes, 0, K, P(i32["root"]), P(i32["size"]), stream) == 0
    assert L.gs_room_table(P(label), P(cost), *dims, P(i32["root"]), 0, P(i32["size"]), P(i32["core_size"]), P(total),
                           P(i32["bbox"]), P(i32["reach"]), stream) == 0
    assert L.gs_room_door_table(P(open_), P(label), P(door), None, *dims, P(i32["root"]), 0, P(i32["size"]), P(total),
                                P(i32["bbox"]), P(i32["lo"]), P(i32["hi"]), P(widest), stream) == 0
    torch.cuda.synchronize()
    for t in everything:
        assert (t == 113).all()


# ---- end to end on a hand-built volume ----------------------------------------------------------------------------------
VOXEL, ROOM, WALL_X, DOOR_Y, DOOR_Z = GG.VOXEL, GG.ROOM, GG.WALL_X, GG.DOOR_Y, GG.DOOR_Z


room = GG.room                                              # test_geodesic_gpu's fixture, built once for this module


def test_esdf_rooms_finds_two_rooms_and_the_door_between_them(built_lib, room):
    from go_slam_amd import rooms
    vol, field = room
    radius, core_radius = VOXEL, 4 * VOXEL                  # the door is 8 points wide: none is > 4 voxels from a jamb
    seg = field.rooms(robot_radius=radius, core_radius=core_radius)
    open_, core = field.passable(radius).cpu().numpy(), field.passable(core_radius).cpu().numpy()
    d2 = field.d2.cpu().numpy()
    ref = RR.segments(open_, core, d2)
    assert_segments(seg, ref)
    print("rooms", ref["rooms"]["size"].tolist(), "doors", ref["doors"]["size"].tolist(), "sweeps", seg.sweeps)
    assert seg.n_rooms == 2 and seg.n_doors == 1 and seg.graph()["doors"] == [(0, 1)]
    assert seg.room_at((8, 6, 30)) == 0 and seg.room_at((33, 16, 6)) == 1
    # the doorway lies in the opening, and its width is that of the opening
    bbox = seg.doors["bbox"][0].cpu().tolist()
    assert WALL_X[0] - 2 <= bbox[0] and bbox[3] <= WALL_X[1] + 2
    assert DOOR_Y[0] <= bbox[1] and bbox[4] <= DOOR_Y[1] and DOOR_Z[0] <= bbox[2] and bbox[5] <= DOOR_Z[1]
    width = float(seg.door_width_m[0])
    built = (DOOR_Z[1] - DOOR_Z[0]) * VOXEL                 # between the opening's outermost free lattice points
    print("width_m", width, "built", built)
    assert abs(width - built) <= VOXEL
    centre = seg.door_centre[0].cpu().numpy() / VOXEL       # lo = 0
    assert WALL_X[0] - 2 <= centre[0] <= WALL_X[1] + 2 and DOOR_Z[0] + 2 <= centre[2] <= DOOR_Z[1] - 2
    assert width == 2.0 * math.sqrt(float(ref["doors"]["widest_d2"][0])) * VOXEL
    # world-space extras
    cells = ref["rooms"]["sum"].astype(np.float64) / ref["rooms"]["size"].astype(np.float64)[:, None]
    assert np.array_equal(seg.centroid.cpu().numpy(), cells * VOXEL)
    assert np.array_equal(seg.volume_m3.cpu().numpy(), ref["rooms"]["size"].astype(np.float64) * VOXEL ** 3)
    assert np.array_equal(seg.box_lo.cpu().numpy(), ref["rooms"]["bbox"][:, :3].astype(np.float64) * VOXEL)
    assert np.array_equal(seg.box_hi.cpu().numpy(), ref["rooms"]["bbox"][:, 3:].astype(np.float64) * VOXEL)
    # the planned path from one room to the other reads room, door, room
    res = field.plan(GG.START, GG.GOAL, robot_radius=radius)
    assert res["reachable"]
    along = seg.rooms_along(res["cells"])
    assert along["rooms"] == [0, 1] and along["doors"] == [0] and sum(along["cells"]) == int(res["cells"].shape[0])
    # map/rooms.txt of it, with a box in each room and one inside the wall
    boxes = [{"centre": np.array(GG.START), "size_m": np.array([0.2, 0.2, 0.2])},
             {"centre": np.array(GG.GOAL), "size_m": np.array([0.2, 0.2, 0.2])},
             {"centre": np.array([0.0, 0.0, 0.0]), "size_m": np.array([0.1, 0.1, 0.1])}]
    report = rooms.parse_rooms(rooms.rooms_text(seg, boxes, along, rooms.room_of_point(seg, GG.GOAL)))
    assert report["object_rooms"] == [0, 1, -1] and report["along_rooms"] == [0, 1] and report["camera_room"] == 1
    assert report["n_rooms"] == 2 and report["doors"]["width_m"][0] == width
    assert np.array_equal(report["rooms"]["volume_m3"], seg.volume_m3.cpu().numpy())
    # a least core larger than the smaller half leaves one room; a core radius that fits the door merges them
    big = int(ref["rooms"]["core_size"].min()) + 1
    assert field.rooms(robot_radius=radius, core_radius=core_radius, min_core_cells=big).n_doors == 0
    assert field.rooms(robot_radius=radius, core_radius=2 * VOXEL).n_rooms == 1


def test_rooms_on_map_finds_the_same_door(built_lib, room):
    from go_slam_amd import rooms
    vol, field = room
    grid = field.occupancy_slice(1, (6 * VOXEL, 8 * VOXEL), robot_radius=VOXEL)
    core_grid = field.occupancy_slice(1, (6 * VOXEL, 8 * VOXEL), robot_radius=4 * VOXEL)
    seg = rooms.rooms_on_map(grid, core_grid)
    free, core = grid["cells"].cpu().numpy() == 254, core_grid["cells"].cpu().numpy() == 254
    ref = RR.segments(free[None], core[None])
    assert_segments(seg, ref)
    assert seg.n_rooms == 2 and seg.n_doors == 1
    assert np.array_equal(seg.area_m2.cpu().numpy(), ref["rooms"]["size"].astype(np.float64) * VOXEL ** 2)
    cells = ref["rooms"]["sum"].astype(np.float64)[:, 1:] / ref["rooms"]["size"].astype(np.float64)[:, None]
    assert np.array_equal(seg.centroid.cpu().numpy(), np.array(grid["origin"]) + (cells + 0.5) * VOXEL)
    assert rooms.rooms_on_map(grid, core_grid, min_core_cells=int(ref["rooms"]["core_size"].max()) + 1).n_rooms == 0


# ---- whole run ----------------------------------------------------------------------------------------------------------
def test_only_tracking_run_ends_with_a_rooms_file(built_lib, tmp_path, monkeypatch):
    from go_slam_amd import rooms
    from go_slam_amd.slam import SLAM
    returned = []
    terminate = SLAM.terminate

    def keeping(self, *args, **kw):
        returned.append(terminate(self, *args, **kw))
        return returned[-1]
    monkeypatch.setattr(SLAM, "terminate", keeping)
    out_dir = str(tmp_path / "with")
    esdf_cfg = {"enable": True, "max_distance": 1.0, "slice": {"up_axis": 1, "height": [-0.5, 0.5], "robot_radius": 0.2},
                "plan": {"enable": True, "robot_radius": 0.2, "snap": 1.0, "allow_unknown": True, "goal": [0.6, 0.0, 0.3]},
                "rooms": {"enable": True, "robot_radius": 0.2, "core_radius": 0.4, "min_core_m3": 0.002, "snap": 1.0}}
    EG.TG.whole_run(out_dir, {"enable": True, "source": "sensor", "voxel_size": 0.1, "esdf": esdf_cfg})
    stats = returned[0]
    report = rooms.parse_rooms(open(f"{out_dir}/map/rooms.txt").read())
    print("map/rooms.txt:", {k: report[k] for k in rooms.SUMMARY_ORDER})
    assert stats["tsdf_rooms_found"] == report["n_rooms"] == len(report["rooms"]["id"])
    assert stats["tsdf_doors_found"] == report["n_doors"] == len(report["doors"]["id"])
    assert report["n_open"] >= report["n_core"] >= 0 and report["object_rooms"] is None
    assert report["rooms"]["size"].sum() <= report["n_open"] and (report["rooms"]["core_size"] >= 2).all()
    assert np.array_equal(report["rooms"]["volume_m3"], report["rooms"]["size"].astype(np.float64) * 0.1 ** 3)
    assert report["camera_room"] is not None and -1 <= report["camera_room"] < max(report["n_rooms"], 1)
    assert (report["along_rooms"] is not None) == stats["tsdf_path_reachable"]
    assert os.path.join("map", "rooms.txt") in EG.TG.listing(out_dir)
