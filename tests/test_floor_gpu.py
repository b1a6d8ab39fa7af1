"""The drivable-floor kernels on the MI355X (csrc/floor.hip, go_slam_amd/floor.py, ESDF.floor_map): both equal the numpy
restatement (tests/floor_restatement.py) with torch.equal into sentinel-filled outputs -- the columns kernel for every up
axis and sign, the footprint up to the halo cap --, the C entries refuse bad arguments before anything is written,
ESDF.floor_map on the hand-built scene goes through plan_on_map and floor.lift, two runs give equal bits, and an
only-tracking run with tsdf.esdf.floor ends with the map, map/floor.txt and map/floor_path.txt."""
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import floor_restatement as R                                  # noqa: E402
import test_esdf_gpu as EG                                     # noqa: E402  (its only-tracking run)
import test_floor_cpu as FC                                    # noqa: E402  (the hand-built scene, once)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INVALID = -1
_REF = {}


def gpu(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)  # a copy: the shared references are read-only


# up along the last axis; the tall one walks three 64-position tiles of the z path (a choice of this file: the contract's
# lattices stay within one)
LATTICES = {"17x15x9": (17, 15, 9), "33x31x12": (33, 31, 12), "64x5x7": (64, 5, 7), "scene": FC.SCENE_DIMS,
            "6x5x150": (6, 5, 150)}


def base_lattice(name):
    if name not in _REF:
        if name == "scene":
            s = FC.scene_state()
        else:
            rng = np.random.default_rng(sum(LATTICES[name]))
            s = rng.integers(0, 3, LATTICES[name]).astype(np.uint8)          # each state at probability 1/3
            if name == "6x5x150":                              # long runs too: stands whose headroom crosses tiles
                s[::2] = np.repeat(rng.integers(0, 3, (3, 5, 10)), 15, axis=2).astype(np.uint8)
            s.setflags(write=False)
        _REF[name] = s
    return _REF[name]


def bands(n):
    """Touching the bottom (no stand is possible at 0), touching the top, a single layer."""
    return [(0, min(2, n - 1)), (max(n - 3, 0), n - 1), (n // 2, n // 2)]


@pytest.mark.parametrize("up_sign", [1, -1])
@pytest.mark.parametrize("up_axis", [0, 1, 2])
@pytest.mark.parametrize("name", list(LATTICES))
def test_columns_equal_the_restatement(built_lib, name, up_axis, up_sign):
    from go_slam_amd import floor as F
    base = base_lattice(name)
    n = base.shape[2]
    state = np.ascontiguousarray(np.moveaxis(base[:, :, ::up_sign], 2, up_axis))
    dstate = gpu(state)
    shape = tuple(d for a, d in enumerate(state.shape) if a != up_axis)
    kinds = _REF.setdefault("kinds", {})
    for H in (1, 3, 8, n + 5):
        for p0, p1 in bands(n) + ([(0, n - 1)] if name == "6x5x150" else []):
            want_floor, want_kind = R.columns(state, up_axis, up_sign, p0, p1, H)
            floor = torch.full(shape, -7, dtype=torch.int16, device=DEV)
            kind = torch.full(shape, 99, dtype=torch.uint8, device=DEV)
            got = F.columns(dstate, up_axis, up_sign, p0, p1, H, out=(floor, kind))
            assert got[0] is floor and got[1] is kind
            assert torch.equal(kind.cpu(), torch.from_numpy(want_kind)), (H, p0, p1)
            assert torch.equal(floor.cpu(), torch.from_numpy(want_floor)), (H, p0, p1)
            kinds.setdefault(name, set()).update(np.unique(want_kind).tolist())
    assert kinds[name] == {0, 1, 2, 3}, kinds[name]


def test_columns_give_the_same_bits_for_every_axis_and_run(built_lib):
    from go_slam_amd import floor as F
    base = base_lattice("33x31x12")
    first = None
    for up_axis in (0, 1, 2):
        for up_sign in (1, -1):
            state = gpu(np.moveaxis(base[:, :, ::up_sign], 2, up_axis))
            floor, kind = F.columns(state, up_axis, up_sign, 1, 8, 3)
            again = F.columns(state, up_axis, up_sign, 1, 8, 3)
            assert torch.equal(floor, again[0]) and torch.equal(kind, again[1])
            position = torch.where(floor < 0, floor, floor if up_sign > 0 else 11 - floor)
            if first is None:
                first = (position, kind)
            assert torch.equal(position, first[0]) and torch.equal(kind, first[1]), (up_axis, up_sign)


def footprint_map(shape, open_):
    """(floor, kind): plateaus one cell apart with bumps; `open_`: every column a floor (the border is drivable but for
    the off-map rule), else one column in eight of another kind."""
    key = ("map", shape, open_)
    if key not in _REF:
        rng = np.random.default_rng(shape[0] * 7 + shape[1] + open_)
        floor = (3 + np.arange(shape[0])[:, None] // 9 + (rng.random(shape) < 0.03) * rng.integers(-3, 5, shape)).astype(np.int16)
        kind = np.ones(shape, dtype=np.uint8)
        if not open_:
            kind = rng.choice(np.array([0, 1, 2, 3], dtype=np.uint8), size=shape, p=[0.04, 0.88, 0.04, 0.04])
            floor[(kind == 0) | (kind == 3)] = -1
        floor.setflags(write=False)
        kind.setflags(write=False)
        _REF[key] = (floor, kind)
    return _REF[key]


@pytest.mark.parametrize("open_", [True, False])
@pytest.mark.parametrize("shape", [(17, 15), (16, 16), (33, 31), (80, 3)])
def test_footprint_equals_the_restatement(built_lib, shape, open_):
    from go_slam_amd import floor as F
    floor, kind = footprint_map(shape, open_)
    dfloor, dkind = gpu(floor), gpu(kind)
    seen, reasons = set(), set()
    for R2 in (2, 3, 9, 10, 25, 1024):
        scan = R.footprint_scan(floor, kind, R2)
        for S in (0, 1, 3):
            want = R.footprint_rules(kind, scan, S)
            out = (torch.full(shape, 77, dtype=torch.uint8, device=DEV), torch.full(shape, 77, dtype=torch.uint8, device=DEV),
                   torch.full(shape, -7, dtype=torch.int16, device=DEV))
            got = F.footprint(dfloor, dkind, R2, S, out=out)
            assert all(g is o for g, o in zip(got, out))
            for name, g, w in zip(("cells", "why", "rough"), got, want):
                assert torch.equal(g.cpu(), torch.from_numpy(w)), (name, R2, S)
            seen |= set(np.unique(want[0]).tolist())
            reasons |= set(np.unique(want[1]).tolist())
            if open_ and R2 == 2 and S == 3:                   # the off-map rule alone keeps the border from being free
                border = np.ones(shape, dtype=bool)
                border[1:-1, 1:-1] = False
                assert (want[0][border] != 254).all() and (want[0][border] == 205).any() and (want[0][~border] == 254).any()
    assert seen == {0, 205, 254} and reasons == ({0, 3} if open_ else {0, 1, 2, 3})


def test_footprint_of_the_scene_and_two_runs(built_lib):
    from go_slam_amd import floor as F
    state = gpu(FC.scene_state())
    for H, S in ((5, 0), (5, 1), (8, 1), (14, 3)):
        floor, kind = F.columns(state, 2, 1, 1, 7, H)
        want_floor, want_kind = R.columns(FC.scene_state(), 2, 1, 1, 7, H)
        assert torch.equal(floor.cpu(), torch.from_numpy(want_floor)) and torch.equal(kind.cpu(), torch.from_numpy(want_kind))
        got = F.footprint(floor, kind, 2, S)
        again = F.footprint(floor, kind, 2, S)
        for g, a, w in zip(got, again, R.footprint(want_floor, want_kind, 2, S)):
            assert torch.equal(g, a) and torch.equal(g.cpu(), torch.from_numpy(w)), (H, S)


def test_c_abi_refusals_leave_the_outputs_untouched(built_lib):
    from go_slam_amd import _lib
    L, P = _lib.lib(), _lib.ptr
    stream = _lib.stream_ptr(DEV)
    state = torch.ones((6, 5, 4), dtype=torch.uint8, device=DEV)
    floor = torch.full((6, 5), -7, dtype=torch.int16, device=DEV)
    kind = torch.full((6, 5), 99, dtype=torch.uint8, device=DEV)
    good = dict(state=P(state), nx=6, ny=5, nz=4, up_axis=2, up_sign=1, p0=1, p1=2, H=2, floor=P(floor), kind=P(kind))
    bad = [("state", None), ("floor", None), ("kind", None), ("nx", 1), ("ny", 1025), ("nz", -1), ("nz", 1), ("up_axis", 3),
           ("up_axis", -1), ("up_sign", 0), ("up_sign", 2), ("up_sign", -2), ("p0", -1), ("p0", 3), ("p1", 4), ("p1", 0),
           ("H", 0), ("H", -5)]
    for key, value in bad:
        assert L.gs_floor_columns(*{**good, key: value}.values(), stream) == INVALID, (key, value)
    assert b"floor_columns" in L.gs_last_error()
    assert L.gs_floor_columns(*{**good, "up_axis": 0, "p1": 6}.values(), stream) == INVALID      # axis 0 has six positions
    cells = torch.full((6, 5), 77, dtype=torch.uint8, device=DEV)
    why = torch.full((6, 5), 77, dtype=torch.uint8, device=DEV)
    rough = torch.full((6, 5), -7, dtype=torch.int16, device=DEV)
    in_floor = torch.zeros((6, 5), dtype=torch.int16, device=DEV)
    in_kind = torch.ones((6, 5), dtype=torch.uint8, device=DEV)
    good2 = dict(floor=P(in_floor), kind=P(in_kind), n_u=6, n_v=5, R2=2, S=0, cells=P(cells), why=P(why), rough=P(rough))
    bad2 = [("floor", None), ("kind", None), ("cells", None), ("why", None), ("rough", None), ("n_u", 1), ("n_u", 1025),
            ("n_v", 0), ("n_v", 1025), ("R2", 1), ("R2", 0), ("R2", -1), ("R2", 1025), ("S", -1)]
    for key, value in bad2:
        assert L.gs_floor_footprint(*{**good2, key: value}.values(), stream) == INVALID, (key, value)
    assert b"floor_footprint" in L.gs_last_error()
    torch.cuda.synchronize()
    assert bool((floor == -7).all()) and bool((kind == 99).all()) and bool((cells == 77).all())
    assert bool((why == 77).all()) and bool((rough == -7).all())
    assert L.gs_floor_columns(*good.values(), stream) == 0 and L.gs_floor_footprint(*good2.values(), stream) == 0
    torch.cuda.synchronize()
    assert bool((kind == 3).all()) and bool((floor == -1).all())             # all free: seen to the bottom, no support
    assert bool((cells[1:-1, 1:-1] == 254).all()) and bool((why == 0).all()) and bool((rough == 0).all())


def scene_field():
    from go_slam_amd import tsdf
    state = gpu(FC.scene_state())
    dims = FC.SCENE_DIMS
    return tsdf.ESDF(state, torch.full(dims, 4, dtype=torch.int32, device=DEV),
                     torch.full(dims, 0.1, dtype=torch.float32, device=DEV), [-0.5, 0.25, -0.1], FC.VOXEL, dims, 3)


def test_floor_map_plans_and_lifts_over_the_step(built_lib):
    from go_slam_amd import floor as F, plan
    field = scene_field()
    lo, vx = field.lo, FC.VOXEL
    height = (lo[2] + 0.9 * vx, lo[2] + 7.1 * vx)              # the layers 1 .. 7
    start = (lo[0] + 4 * vx, lo[1] + 8 * vx)
    goal = (lo[0] + 20 * vx, lo[1] + 10 * vx)
    for step_height, S in ((0.0, 0), (0.06, 1), (0.16, 3)):
        grid = field.floor_map(2, height, robot_radius=0.08, robot_height=0.24, step_height=step_height)
        again = field.floor_map(2, height, robot_radius=0.08, robot_height=0.24, step_height=step_height)
        want_floor, want_kind = R.columns(FC.scene_state(), 2, 1, 1, 7, 5)
        want = R.footprint(want_floor, want_kind, 2, S)
        for key, w in zip(("floor", "kind", "cells", "why", "rough"), (want_floor, want_kind) + want):
            assert torch.equal(grid[key].cpu(), torch.from_numpy(w)), (key, S)
            assert torch.equal(grid[key], again[key])
        assert grid["axes"] == (0, 1) and grid["up_axis"] == 2 and grid["up_sign"] == 1 and grid["resolution"] == vx
        assert grid["origin"] == (float(lo[0] - 0.5 * vx), float(lo[1] - 0.5 * vx))
        fh = grid["floor_height"].cpu().numpy()
        assert fh.dtype == np.float32 and np.array_equal(np.isnan(fh), want_floor < 0)
        assert np.array_equal(fh[want_floor >= 0], (lo[2] + (want_floor[want_floor >= 0].astype(np.float64) - 0.5) * vx).astype(np.float32))
        route = plan.plan_on_map(grid, start, goal)
        assert route["start_cell"] == (4, 8) and route["goal_cell"] == (20, 10)
        assert route["reachable"] == (S >= 1), S               # the one-cell step (and the foot of the ramp) need S >= 1
        if not route["reachable"]:
            assert tuple(F.lift(grid, route["cells"]).shape) == (0, 3)
            continue
        cells = route["cells"].cpu().numpy()
        assert (want[0][cells[:, 0], cells[:, 1]] == 254).all()
        pts = F.lift(grid, route["cells"])
        assert pts.dtype == torch.float64 and pts.device == route["cells"].device and tuple(pts.shape) == (len(cells), 3)
        pts = pts.cpu().numpy()
        assert np.array_equal(pts[:, :2], route["points"].cpu().numpy())
        assert np.array_equal(pts[:, 2], fh[cells[:, 0], cells[:, 1]].astype(np.float64))
        assert pts[0, 2] == float(np.float32(lo[2] + 1.5 * vx)) and pts[-1, 2] == float(np.float32(lo[2] + 2.5 * vx))
        assert np.abs(np.diff(want_floor[cells[:, 0], cells[:, 1]].astype(np.int64))).max() <= S    # no move climbs more than S
        with pytest.raises(ValueError, match="has no floor"):
            F.lift(grid, [[4, 8], [10, 10]])
    # the same scene with up along -x: the lattice turned, the map's bits stay
    turned = gpu(np.moveaxis(FC.scene_state()[:, :, ::-1], 2, 0))
    from go_slam_amd import tsdf
    dims = tuple(turned.shape)
    other = tsdf.ESDF(turned, field.d2.new_zeros(dims), field.dist.new_zeros(dims), [-0.1, -0.5, 0.25], vx, dims, 3)
    top = -0.1 + 15 * vx
    flipped = other.floor_map(0, (top - 7.1 * vx, top - 0.9 * vx), 0.08, 0.24, 0.06, up_sign=-1)
    grid = field.floor_map(2, height, 0.08, 0.24, 0.06)
    for key in ("cells", "kind", "why", "rough"):
        assert torch.equal(flipped[key], grid[key]), key
    assert torch.equal(torch.where(flipped["floor"] < 0, flipped["floor"], 15 - flipped["floor"]), grid["floor"])
    assert flipped["axes"] == (1, 2) and flipped["up_sign"] == -1
    k = flipped["floor"][4, 8].item()
    assert k == 13 and float(flipped["floor_height"][4, 8]) == float(np.float32(-0.1 + (k + 0.5) * vx))


def test_only_tracking_run_ends_with_the_floor_files(built_lib, tmp_path, monkeypatch):
    from go_slam_amd import floor as F, plan, tsdf
    from go_slam_amd.slam import SLAM
    returned = []
    terminate = SLAM.terminate

    def keeping(self, *args, **kw):
        returned.append(terminate(self, *args, **kw))
        return returned[-1]
    monkeypatch.setattr(SLAM, "terminate", keeping)
    out = str(tmp_path / "with")
    floor_cfg = {"enable": True, "up_axis": 1, "up_sign": -1, "height": [-3.0, 2.0], "robot_radius": 0.15,
                 "robot_height": 0.3, "step_height": 0.1, "plan": True}
    cfg = {"enable": True, "source": "sensor", "voxel_size": 0.1,
           "esdf": {"enable": True, "max_distance": 1.0, "floor": floor_cfg,
                    "plan": {"enable": True, "robot_radius": 0.2, "snap": 1.0, "allow_unknown": True, "goal": [0.6, 0.0, 0.3]}}}
    EG.TG.whole_run(out, cfg)
    stats = returned[0]
    report = F.parse_floor(open(f"{out}/map/floor.txt").read())
    print("map/floor.txt:", report)
    assert stats["tsdf_floor_map_drivable_m2"] == report["drivable_m2"]
    assert stats["tsdf_floor_map_unknown_m2"] == report["unknown_m2"]
    grid = tsdf.load_map(f"{out}/map/floor")
    counts = {v: int((grid["cells"] == v).sum()) for v in (254, 0, 205)}
    assert sum(counts.values()) == grid["cells"].size and grid["resolution"] == 0.1
    area = 0.1 ** 2
    assert (report["drivable_m2"], report["blocked_m2"], report["unknown_m2"]) == \
        (counts[254] * area, counts[0] * area, counts[205] * area)
    assert report["blocked_no_floor"] + report["blocked_near_no_floor"] + report["blocked_step"] == counts[0]
    head, pts = plan.parse_path(open(f"{out}/map/floor_path.txt").read())
    assert head["reachable"] == stats["tsdf_floor_path_reachable"] and head["n_points"] == len(pts)
    assert math.isnan(head["min_clearance_m"]) and (head["length_m"] == stats["tsdf_floor_path_length_m"] or not head["reachable"])
    listed = EG.TG.listing(out)
    for name in ("floor.txt", "floor_path.txt", os.path.join("floor", "occupancy.pgm"), os.path.join("floor", "occupancy.yaml"),
                 "path.txt"):
        assert os.path.join("map", name) in listed, name
