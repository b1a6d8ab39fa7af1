"""The room restatement (tests/rooms_restatement.py) judged without a GPU: its components against scipy.ndimage, its
labels against an independent brute force (one Dijkstra field per core), the properties the definitions promise, a hand
plan with known rooms and doorways and a tie; map/rooms.txt's writer and reader, the refusals that need no device, and the
resources of csrc/rooms.hip's kernels."""
import math
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import geodesic_restatement as GR                              # noqa: E402
import rooms_restatement as RR                                 # noqa: E402
from go_slam_amd import rooms, tsdf                            # noqa: E402

INF = GR.INF
FULL = np.ones((3, 3, 3), dtype=bool)
_REF = {}


# ---- the lattices (tests/test_rooms_gpu.py runs the same ones on the device) --------------------------------------------
def hand_plan(open_above=2, core_above=6):
    """The 40 x 64 plan as the lattice [1,40,64]: (open, core, d2).  All wall except rows 2..37 of columns 2..29 and of
    columns 32..61; a door at rows 6..14 of columns 30..31 joins the halves; a wall across rows 20..21 of the right half is
    pierced at columns 44..51.  d is the exact Euclidean distance to the nearest wall cell."""
    free = np.zeros((40, 64), dtype=bool)
    free[2:38, 2:30] = True
    free[2:38, 32:62] = True
    free[6:15, 30:32] = True
    free[20:22, 32:62] = False
    free[20:22, 44:52] = True
    d = ndimage.distance_transform_edt(free)
    d2 = np.rint(d * d).astype(np.int32)                    # exact: d^2 is an integer
    return (d > open_above)[None], (d > core_above)[None], d2[None]


def random_lattice(seed=0, dims=(9, 13, 70)):
    rng = np.random.default_rng(seed)
    open_ = rng.random(dims) < 0.8
    core = open_ & (rng.random(dims) < 0.02)
    d2 = rng.integers(0, 50, dims).astype(np.int32)
    return open_, core, d2


def small_lattice(seed):
    """At most 600 cells, a handful of cores."""
    rng = np.random.default_rng(seed)
    dims = (4, 9, 16)
    open_ = rng.random(dims) < 0.8
    core = open_ & (rng.random(dims) < 0.08)
    return open_, core


def corridor():
    """[1,3,41], a core at each end: the middle column is equidistant."""
    open_ = np.ones((1, 3, 41), dtype=bool)
    core = np.zeros_like(open_)
    core[0, :, 0] = core[0, :, 40] = True
    return open_, core


def reference(name, open_, core, d2=None, min_core_cells=1, max_cost=GR.MAX_COST):
    """The restatement's result, computed once per named case and left unchanged."""
    key = (name, d2 is not None, min_core_cells, max_cost)
    if key not in _REF:
        _REF[key] = RR.segments(open_, core, d2, min_core_cells, max_cost)
        for v in _REF[key].values():
            for a in (v.values() if isinstance(v, dict) else [v]):
                a.setflags(write=False)
    return _REF[key]


def roots_of(label_image):
    """scipy's components as our labels: -1 off them, else the smallest linear index."""
    out = np.full(label_image.shape, -1, dtype=np.int32)
    lin = np.arange(label_image.size).reshape(label_image.shape)
    for k in range(1, int(label_image.max()) + 1):
        out[label_image == k] = lin[label_image == k].min()
    return out


# ---- the restatement against independent answers --------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["hand", "random"])
def test_components_and_doorways_equal_scipy(case):
    open_, core, d2 = hand_plan() if case == "hand" else random_lattice()
    ref = reference(case, open_, core, d2)
    truth = roots_of(ndimage.label(open_ & core, structure=FULL)[0])
    kept = np.where(ref["cost"] == 0, ref["label"], -1)
    assert np.array_equal(kept, truth)                      # min_core_cells = 1: every core is kept
    ok = GR.move_masks(open_)
    boundary = np.zeros(open_.shape, dtype=bool)
    for c in np.ndindex(*open_.shape):
        boundary[c] = ref["label"][c] >= 0 and len(RR.across(ok, ref["label"], c)) > 0
    assert np.array_equal(ref["door_label"], roots_of(ndimage.label(boundary, structure=FULL)[0]))
    assert ref["counts"].tolist() == [open_.sum(), (open_ & core).sum(), boundary.sum()]


def brute_labels(open_, core_label, max_cost=GR.MAX_COST):
    """One Dijkstra field per kept core; a cell's label is the smallest root among the cores whose field equals the
    minimum there."""
    roots = sorted(set(int(v) for v in core_label.ravel() if v >= 0))
    fields = np.stack([GR.field(open_, np.argwhere(core_label == r), max_cost) for r in roots]) if roots else None
    label = np.full(open_.shape, -1, dtype=np.int32)
    if roots:
        best = fields.min(axis=0)
        for i in reversed(range(len(roots))):               # descending: the smallest root is written last
            label[(fields[i] == best) & (best < INF)] = roots[i]
    return label, (fields.min(axis=0) if roots else np.full(open_.shape, INF, dtype=np.int32))


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("min_core_cells", [1, 2])
def test_labels_equal_a_brute_force_over_one_field_per_core(seed, min_core_cells):
    open_, core = small_lattice(seed)
    assert open_.size <= 600
    ref = RR.segments(open_, core, None, min_core_cells)
    core_label, _, sizes = RR.kept_cores(open_, core, min_core_cells)
    want, cost = brute_labels(open_, core_label)
    print("cores", len(sizes), "kept", len(ref["rooms"]["root"]), "labelled", int((want >= 0).sum()))
    assert len(ref["rooms"]["root"]) >= 2
    assert np.array_equal(ref["cost"], cost) and np.array_equal(ref["label"], want)


def check_properties(open_, ref):
    label, cost = ref["label"], ref["cost"]
    ok = GR.move_masks(open_)
    # every room is connected under allowed moves
    for r in ref["rooms"]["root"]:
        inside = label == r
        start = tuple(int(v) for v in np.unravel_index(int(r), label.shape))
        seen, stack = {start}, [start]
        while stack:
            c = stack.pop()
            for m, d in enumerate(GR.MOVES):
                q = (c[0] + d[0], c[1] + d[1], c[2] + d[2])
                if ok[(m,) + c] and inside[q] and q not in seen:
                    seen.add(q)
                    stack.append(q)
        assert len(seen) == int(inside.sum()), f"room {r} is not connected"
    # every labelled non-core cell has a parent with its own label
    for c in np.argwhere((label >= 0) & (cost > 0)):
        c = tuple(int(v) for v in c)
        parents = []
        for m, (d, w) in enumerate(zip(GR.MOVES, GR.WEIGHTS)):
            q = (c[0] + d[0], c[1] + d[1], c[2] + d[2])
            if ok[(m,) + c] and int(cost[q]) + w == int(cost[c]):
                parents.append(int(label[q]))
        assert parents and min(parents) == label[c]
    assert ((label >= 0) == (open_ & (cost < INF))).all()
    # the tables say what the lattices say
    for i, r in enumerate(ref["rooms"]["root"]):
        cells = np.argwhere(label == r)
        assert ref["rooms"]["size"][i] == len(cells) and ref["rooms"]["reach"][i] == cost[label == r].max()
        assert ref["rooms"]["core_size"][i] == ((label == r) & (cost == 0)).sum()
        assert ref["rooms"]["sum"][i].tolist() == cells.sum(axis=0).tolist()
        assert ref["rooms"]["bbox"][i].tolist() == cells.min(axis=0).tolist() + cells.max(axis=0).tolist()


@pytest.mark.parametrize("case", ["hand", "random"])
def test_rooms_are_connected_and_every_cell_has_a_parent_of_its_label(case):
    open_, core, d2 = hand_plan() if case == "hand" else random_lattice()
    check_properties(open_, reference(case, open_, core, d2))


def test_hand_plan_has_three_rooms_and_two_doorways():
    open_, core, d2 = hand_plan()
    ref = reference("hand", open_, core, d2)
    rooms_, doors = ref["rooms"], ref["doors"]
    assert rooms_["size"].tolist() == [789, 403, 330] and doors["size"].tolist() == [10, 8]
    assert int((open_ & (ref["label"] < 0)).sum()) == 0                    # no open cell unlabelled
    left, upper, lower = (int(r) for r in rooms_["root"])
    assert np.unravel_index(left, open_.shape)[2] < 30 < np.unravel_index(upper, open_.shape)[2]
    assert np.unravel_index(lower, open_.shape)[1] > 21
    assert doors["room_lo"].tolist() == [left, upper] and doors["room_hi"].tolist() == [upper, lower]
    # the doorways lie in the openings, and the widest cell of each has the opening's clearance
    for i, (rows, cols) in enumerate((((6, 14), (28, 34)), ((18, 23), (44, 51)))):
        b = doors["bbox"][i]
        assert rows[0] <= b[1] and b[4] <= rows[1] and cols[0] <= b[2] and b[5] <= cols[1], b
        cells = np.argwhere(ref["door_label"] == doors["root"][i])
        best = max(int(d2[tuple(c)]) for c in cells)
        first = min(int(np.ravel_multi_index(tuple(c), open_.shape)) for c in cells if d2[tuple(c)] == best)
        assert doors["widest_d2"][i] == best and doors["widest_cell"][i] == first
    assert doors["widest_d2"].tolist() == [25, 16]          # a 9-cell and an 8-cell opening: d = 5 and 4 at their middles
    # without d2 the widest cell is the doorway's root
    plain = reference("hand", open_, core, None)
    assert plain["doors"]["widest_cell"].tolist() == plain["doors"]["root"].tolist()
    assert plain["doors"]["widest_d2"].tolist() == [0, 0]

    # a smaller core radius: the door's middle is core and merges the left and the upper right room
    open4, core4, _ = hand_plan(1, 4)
    merged = reference("hand 1 4", open4, core4)
    assert len(merged["rooms"]["root"]) == 2 and len(merged["doors"]["root"]) == 1
    assert core4[0, 10, 30] and merged["label"][0, 10, 10] == merged["label"][0, 10, 50] != merged["label"][0, 30, 50]
    # only the left room's core has 200 cells
    sizes = ref["core_sizes"].tolist()
    assert sorted(sizes)[-1] >= 200 > sorted(sizes)[-2]
    one = reference("hand", open_, core, d2, min_core_cells=200)
    assert one["rooms"]["size"].tolist() == [789 + 403 + 330] and len(one["doors"]["root"]) == 0
    assert (one["door_label"] == -1).all() and one["counts"][2] == 0


def test_a_tie_goes_to_the_lower_root():
    open_, core = corridor()
    ref = reference("corridor", open_, core)
    assert ref["rooms"]["root"].tolist() == [0, 40]
    assert (ref["cost"][0, :, 20] == 20000).all()            # 20 straight moves from either end
    assert (ref["label"][0, :, :21] == 0).all() and (ref["label"][0, :, 21:] == 40).all()
    assert ref["rooms"]["size"].tolist() == [63, 60] and ref["rooms"]["core_size"].tolist() == [3, 3]
    assert len(ref["doors"]["root"]) == 1 and ref["doors"]["size"][0] == 6
    assert ref["doors"]["room_lo"][0] == 0 and ref["doors"]["room_hi"][0] == 40


def test_a_cap_leaves_far_cells_without_a_room():
    open_, core = corridor()
    ref = reference("corridor", open_, core, max_cost=5000)
    assert (ref["label"][0, :, 6:35] == -1).all() and (ref["label"][0, :, :6] == 0).all()
    assert len(ref["doors"]["root"]) == 0 and ref["rooms"]["reach"].tolist() == [5000, 5000]


# ---- map/rooms.txt ------------------------------------------------------------------------------------------------------
def test_parse_rooms_inverts_the_writer_bit_for_bit():
    rng = np.random.default_rng(5)
    K, D = 3, 2
    report = {"n_open": 1522, "n_core": 310, "n_boundary": 18, "n_rooms": K, "n_doors": D, "object_rooms": [2, -1, 0],
              "along_rooms": [0, 1], "along_doors": [0], "camera_room": 1,
              "rooms": {c: rng.integers(0, 2 ** 30, K) for c in rooms.ROOM_TEXT_INTS},
              "doors": {c: rng.integers(-1, 2 ** 30, D) for c in rooms.DOOR_TEXT_INTS}}
    report["rooms"].update({c: rng.standard_normal(K) * 10.0 ** rng.integers(-8, 8, K) for c in rooms.ROOM_TEXT_FLOATS})
    report["doors"].update({c: rng.standard_normal(D) / 3.0 for c in rooms.DOOR_TEXT_FLOATS})
    report["doors"]["width_m"] = np.array([2.0 * math.sqrt(25) * 0.05, math.inf])
    text = rooms.rooms_text(report)
    assert text.endswith("\n") and len(text.splitlines()) == 2 + len(rooms.SUMMARY_ORDER) + K + D
    back = rooms.parse_rooms(text)
    for k in rooms.SUMMARY_ORDER:
        assert back[k] == report[k], k
    for table in ("rooms", "doors"):
        assert list(back[table]) == list(report[table])
        for c, v in report[table].items():
            assert back[table][c].dtype == (np.float64 if v.dtype == np.float64 else np.int64)
            assert back[table][c].tobytes() == v.astype(back[table][c].dtype).tobytes(), (table, c)
    assert rooms.rooms_text(back) == text
    nothing = dict(report, n_rooms=0, n_doors=0, object_rooms=None, along_rooms=None, along_doors=None, camera_room=None,
                   rooms={c: np.zeros(0) for c in report["rooms"]}, doors={c: np.zeros(0) for c in report["doors"]})
    back = rooms.parse_rooms(rooms.rooms_text(nothing))
    assert back["object_rooms"] is None and back["camera_room"] is None and back["rooms"]["root"].shape == (0,)
    for bad in ("", "something else\n", text.replace("n_core", "n_cores"), text + "1 2 3\n",
                "\n".join(text.splitlines()[:-1]) + "\n"):
        with pytest.raises(ValueError):
            rooms.parse_rooms(bad)


# ---- refusals that need no GPU --------------------------------------------------------------------------------------------
def test_room_segments_refuses_before_the_device_is_touched(monkeypatch):
    from go_slam_amd import _lib
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was reached"))
    ok = torch.ones(2, 3, 4, dtype=torch.uint8)
    for bad in (ok.float(), ok.int(), ok.numpy()):
        with pytest.raises(ValueError, match="open must be a uint8"):
            rooms.room_segments(bad, ok)
        with pytest.raises(ValueError, match="core must be a uint8"):
            rooms.room_segments(ok, bad)
    for bad in (ok[0], torch.ones(1, 1, 1025, dtype=torch.uint8), torch.ones(0, 2, 2, dtype=torch.uint8)):
        with pytest.raises(ValueError, match=r"\[n0,n1,n2\]"):
            rooms.room_segments(bad, bad)
    with pytest.raises(ValueError, match="core is"):
        rooms.room_segments(ok, torch.ones(2, 3, 5, dtype=torch.uint8))
    with pytest.raises(ValueError, match="d2 must be"):
        rooms.room_segments(ok, ok, d2=ok.long())
    with pytest.raises(ValueError, match="d2 is"):
        rooms.room_segments(ok, ok, d2=torch.zeros(2, 4, 3, dtype=torch.int32))
    for v in (0, -3, 2.0, True):
        with pytest.raises(ValueError, match="min_core_cells"):
            rooms.room_segments(ok, ok, min_core_cells=v)
        with pytest.raises(ValueError, match="max_sweeps"):
            rooms.room_segments(ok, ok, max_sweeps=v)
    for v in (-1, 1.5, True, GR.MAX_COST + 1):
        with pytest.raises(ValueError, match="max_cost"):
            rooms.room_segments(ok, ok, max_cost=v)
    d2 = torch.zeros(2, 3, 4, dtype=torch.int32)
    assert rooms.segment_arguments(ok, ok.bool(), d2, 5, 7000, 9) == ((2, 3, 4), 5, 7000, 9)
    assert rooms.segment_arguments(ok, ok) == ((2, 3, 4), 1, GR.MAX_COST, 65536)


def stub_esdf(dims=(4, 5, 6)):
    state = torch.ones(dims, dtype=torch.uint8)
    return tsdf.ESDF(state, torch.full(dims, 9, dtype=torch.int32), torch.full(dims, 0.3), [0.0, 0.0, 0.0], 0.1, dims, 3)


def test_esdf_rooms_and_rooms_on_map_refuse_before_the_device_is_touched(monkeypatch):
    from go_slam_amd import _lib
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was reached"))
    field = stub_esdf()                                     # a band of 0.3 m
    for robot, core in ((0.2, 0.2), (0.25, 0.1), (0.0, 0.31), (0.0, math.nan), (0.0, 0.0)):
        with pytest.raises(ValueError, match="core_radius"):
            field.rooms(robot_radius=robot, core_radius=core)
    for robot in (-0.1, 0.31, math.nan):
        with pytest.raises(ValueError, match="robot_radius"):
            field.rooms(robot_radius=robot, core_radius=0.3)
    for v in (0.0, -1.0, math.inf, math.nan):
        with pytest.raises(ValueError, match="min_core_m3"):
            field.rooms(core_radius=0.2, min_core_m3=v)
    for v in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="min_core_cells"):
            field.rooms(core_radius=0.2, min_core_cells=v)
    with pytest.raises(ValueError, match="not both"):
        field.rooms(core_radius=0.2, min_core_m3=1.0, min_core_cells=3)
    for v in (0.0, -1.0, math.nan, 1e9):
        with pytest.raises(ValueError, match="max_cost_m"):
            field.rooms(core_radius=0.2, max_cost_m=v)
    assert field.rooms_arguments(0.1, 0.3, min_core_m3=0.0105) == (11, None)        # ceil(0.0105 / 0.001)
    assert field.rooms_arguments(0.0, 0.2, min_core_cells=4, max_cost_m=1.0) == (4, 10000)

    cells = torch.full((4, 6), 254, dtype=torch.uint8)
    grid = {"cells": cells, "origin": (0.0, 1.0), "resolution": 0.1}
    for other in ({**grid, "cells": cells[:3]}, {**grid, "origin": (0.0, 1.1)}, {**grid, "resolution": 0.2}):
        with pytest.raises(ValueError, match="disagree"):
            rooms.rooms_on_map(grid, other)
    with pytest.raises(ValueError, match="uint8"):
        rooms.rooms_on_map({**grid, "cells": cells.float()}, grid)
    with pytest.raises(ValueError, match="resolution"):
        rooms.rooms_on_map({**grid, "resolution": 0.0}, grid)
    with pytest.raises(ValueError, match="min_core_cells"):
        rooms.rooms_on_map(grid, grid, min_core_cells=0)


def test_config_values_are_checked():
    ok = rooms.config_arguments({"enable": True}, 0.1)
    assert ok == {"robot_radius": 0.0, "core_radius": 0.6, "min_core_m3": None, "snap": 0.0}
    assert rooms.config_arguments({"robot_radius": 0.2, "core_radius": 1, "min_core_m3": 0.5, "snap": 1}, 0.1, 1.0) == \
        {"robot_radius": 0.2, "core_radius": 1.0, "min_core_m3": 0.5, "snap": 1.0}
    for bad in ({"robot_radius": 0.6}, {"robot_radius": -0.1}, {"core_radius": "wide"}, {"core_radius": math.nan},
                {"min_core_m3": 0}, {"min_core_m3": -1.0}, {"snap": -1.0}, {"snap": True}, {"radius": 0.2}):
        with pytest.raises(ValueError, match="tsdf.esdf.rooms"):
            rooms.config_arguments(bad, 0.1)
    with pytest.raises(ValueError, match="band"):
        rooms.config_arguments({"core_radius": 0.6}, 0.1, 0.5)


def test_fuse_from_config_refuses_bad_rooms_values_before_anything_is_fused(tmp_path):
    class Slam:
        output = str(tmp_path)
        cfg = {"tsdf": {"enable": True, "voxel_size": 0.1,
                        "esdf": {"enable": True, "max_distance": 1.0,
                                 "rooms": {"enable": True, "robot_radius": 0.5, "core_radius": 0.4}}}}

        @property
        def video(self):
            pytest.fail("the keyframes were reached")
    with pytest.raises(ValueError, match="tsdf.esdf.rooms"):
        tsdf.fuse_from_config(Slam(), c2w_list=[])
    Slam.cfg["tsdf"]["esdf"]["rooms"] = {"enable": True, "core_radius": 1.2}              # beyond max_distance
    with pytest.raises(ValueError, match="band"):
        tsdf.fuse_from_config(Slam(), c2w_list=[])
    assert os.listdir(tmp_path) == []


# ---- the kernels' resources ---------------------------------------------------------------------------------------------
KERNELS = ("room_mark_kernel", "room_emit_kernel", "room_sizes_kernel", "room_seed_kernel", "room_relax_kernel",
           "room_door_mark_kernel", "room_table_init_kernel", "room_table_kernel", "room_door_table_kernel")
BRICK = (4, 4, 32)                                          # frontier_rows.h's, which rooms.hip relaxes on


def test_kernel_resources(tmp_path):
    """test_frontier_cpu.test_kernel_resources for csrc/rooms.hip (compile-only: metadata fields of the gfx950 assembly).
    No kernel uses scratch.  The relax kernel's static LDS is its three tiles -- labels and costs at four bytes and
    passability at one byte per cell of the brick with its halo -- and the skeleton's nine round and face words, each of
    the five arrays padded to at most a 16-byte boundary; that is far below the 20 KB at which LDS would limit the eight
    256-thread workgroups per CU that at most 64 VGPRs allow (eight waves per SIMD, as its two siblings)."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "go_slam_amd", "csrc")
    out = tmp_path / "k.s"
    res = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                          "-fno-gpu-rdc", "-munsafe-fp-atomics", "-I", csrc, "-I", os.path.join(ROOT, "include"),
                          "--cuda-device-only", "-S", os.path.join(csrc, "rooms.hip"), "-o", str(out)],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-2000:]
    tile = (BRICK[0] + 2) * (BRICK[1] + 2) * (BRICK[2] + 2)
    lds_max = 9 * tile + 4 * 9 + 5 * 15
    assert lds_max < 20 * 1024
    pat = re.compile(r"\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.name:\s+(\S+)\n(?:.*\n)*?"
                     r"\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)")
    seen = {}
    for m in pat.finditer(open(out).read()):
        lds, name, scratch, vgpr = int(m.group(1)), m.group(2), int(m.group(3)), int(m.group(4))
        print(name, "VGPRs", vgpr, "LDS", lds, "scratch", scratch)
        assert scratch == 0, f"{name}: {scratch} B of scratch"
        for key in KERNELS:
            if key in name:
                seen[key] = seen.get(key, 0) + 1
        if "room_relax_kernel" in name:
            assert 9 * tile <= lds <= lds_max and vgpr <= 64, f"{name}: {lds} B of LDS, {vgpr} VGPRs"
    assert seen == {k: 1 for k in KERNELS}, seen
