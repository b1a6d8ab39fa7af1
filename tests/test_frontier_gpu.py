"""Frontier cells, their clusters and the cluster table on the MI355X (csrc/frontier.hip, go_slam_amd/frontier.py,
ESDF.frontiers / explore): every output equals the serial restatement (tests/frontier_restatement.py) exactly -- on a
random lattice with a ragged tail and bricks cut on every axis, with and without `open` and `cost`, on a serpentine whose
label has to travel through many bricks, at the smallest sizes, across the corner where eight bricks meet and on the hand
cases; the C ABI refuses bad arguments and writes nothing; a hand-built room whose far half was never observed is explored
end to end; and an only-tracking run with tsdf.esdf.frontiers ends with map/frontiers.txt."""
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import frontier_restatement as FR                              # noqa: E402
import geodesic_restatement as GR                              # noqa: E402
import test_esdf_gpu as EG                                     # noqa: E402  (its only-tracking run)
import test_frontier_cpu as FC                                 # noqa: E402  (the lattices and the hand cases)
import test_geodesic_gpu as GG                                 # noqa: E402  (its room)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INF = FR.INF
_REF = {}


def reference(name, state, open_=None, cost=None):
    """The restatement's result, computed once per named case and left unchanged."""
    if name not in _REF:
        _REF[name] = FR.clusters(state, open_, cost)
        for v in _REF[name].values():
            v.setflags(write=False)
    return _REF[name]


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def gpu_clusters(state, open_=None, cost=None, **kw):
    from go_slam_amd import frontier
    return frontier.frontier_clusters(dev(state), dev(open_), dev(cost), **kw)


def host(fc):
    out = {k: getattr(fc, k).cpu().numpy() for k in ("frontier", "label") + FC.TABLE}
    out["counts"] = fc.counts.cpu().numpy().astype(np.uint32)
    return out


def assert_clusters(fc, ref):
    assert fc.label.dtype == torch.int32 and fc.frontier.dtype == torch.uint8 and fc.sum.dtype == torch.int64
    assert fc.dims == ref["label"].shape and fc.sweeps >= 1 and fc.n_clusters == len(ref["root"])
    FC.assert_same(host(fc), ref)
    want = ref["sum"].astype(np.float64) / ref["size"].astype(np.float64)[:, None]
    assert np.array_equal(fc.centroid_cells().cpu().numpy(), want)


@pytest.mark.parametrize("with_masks", [False, True])
def test_random_lattice_equals_the_restatement(built_lib, with_masks):
    state = FC.random_state()
    open_, cost = FC.random_open_and_cost(state.shape) if with_masks else (None, None)
    ref = reference(f"random {with_masks}", state, open_, cost)
    assert len(ref["root"]) == 64 if not with_masks else len(ref["root"]) > 40            # not vacuous
    fc = gpu_clusters(state, open_, cost)
    print("sweeps", fc.sweeps, "clusters", fc.n_clusters, "frontier cells", int(fc.counts[3]))
    assert_clusters(fc, ref)
    if with_masks:                                          # open alone, cost alone
        assert_clusters(gpu_clusters(state, open_, None), FR.clusters(state, open_, None))
        assert_clusters(gpu_clusters(state, None, cost), FR.clusters(state, None, cost))
        assert_clusters(gpu_clusters(state, open_ != 0, cost), ref)      # a bool mask


def serpentine_state():
    """3 x 17 x 70: test_geodesic_gpu's serpentine as a sheet -- free in layer 1 along the corridors, unknown under
    it in layer 0, solid elsewhere -- so the frontier is one winding component whose lowest index, (1,0,0), is one end."""
    path = GG.serpentine()[1]
    state = np.full((3, 17, 70), 2, dtype=np.uint8)
    state[1][path] = 1
    state[0][path] = 0
    return state


def test_serpentine_needs_more_than_one_sweep_and_max_sweeps_is_an_orderly_error(built_lib):
    from go_slam_amd import frontier
    state = serpentine_state()
    ref = reference("serpentine", state)
    assert len(ref["root"]) == 1 and ref["root"][0] == 17 * 70 and ref["size"][0] == 9 * 70 + 8 * 2
    fc = gpu_clusters(state)
    print("sweeps", fc.sweeps, "brick", frontier.brick())
    assert_clusters(fc, ref)
    assert 1 < fc.sweeps <= 65536
    with pytest.raises(RuntimeError, match="max_sweeps"):
        gpu_clusters(state, max_sweeps=1)
    torch.cuda.synchronize()
    assert_clusters(gpu_clusters(state, max_sweeps=fc.sweeps + 64), ref)     # the device is fine afterwards


@pytest.mark.parametrize("dims", [(1, 1, 1), (1, 5, 7), (2, 2, 2)], ids=lambda d: "x".join(map(str, d)))
def test_smallest_lattices(built_lib, dims):
    rng = np.random.default_rng(sum(dims))
    state = rng.integers(0, 3, size=dims).astype(np.uint8)
    assert_clusters(gpu_clusters(state), FR.clusters(state))
    cost = rng.integers(0, 4, size=dims).astype(np.int32) * 1000
    open_ = (rng.random(dims) > 0.3).astype(np.uint8)
    assert_clusters(gpu_clusters(state, open_, cost), FR.clusters(state, open_, cost))
    for v in (0, 1, 2):                                     # K = 0
        fc = gpu_clusters(np.full(dims, v, dtype=np.uint8))
        assert fc.n_clusters == 0 and int(fc.counts[v]) == int(np.prod(dims)) and int(fc.counts[3]) == 0
        assert (fc.label == -1).all() and fc.root.shape == (0,) and fc.sum.shape == (0, 3) and fc.bbox.shape == (0, 6)
        assert fc.centroid_cells().shape == (0, 3)


def test_a_component_joined_only_through_the_corner_where_eight_bricks_meet(built_lib):
    from go_slam_amd import frontier
    b = frontier.brick()
    dims = tuple(n + 1 for n in b)                          # one brick plus one cell on every axis: 5 x 5 x 33
    state = np.full(dims, 2, dtype=np.uint8)
    a, c = tuple(n - 1 for n in b), b                       # the last cell of brick (0,0,0), the only one of (1,1,1)
    state[a] = state[c] = 1
    state[a[0] - 1, a[1], a[2]] = 0
    state[c[0], c[1] - 1, c[2]] = 0
    ref = FR.clusters(state)
    low = int(np.ravel_multi_index(a, dims))
    assert len(ref["root"]) == 1 and ref["size"][0] == 2 and ref["label"][c] == low
    assert_clusters(gpu_clusters(state), ref)


@pytest.mark.parametrize("case", FC.cases(), ids=lambda c: c[0])
def test_hand_cases(built_lib, case):
    _, state, open_, cost, want = case
    fc = gpu_clusters(state, open_, cost)
    FC.check_want(host(fc), want)
    assert_clusters(fc, FR.clusters(state, open_, cost))


def test_c_abi_bad_arguments_and_table_capacity(built_lib):
    from go_slam_amd import _lib, frontier
    L = _lib.lib()
    P = _lib.ptr
    stream = _lib.stream_ptr(DEV)
    INVALID = -1
    state_h = FC.random_state()
    dims = state_h.shape
    ref = reference("random False", state_h)
    K = len(ref["root"])
    state = dev(state_h)
    n = state_h.size
    GUARD = 16

    def guarded(count, dtype):
        return torch.full((count + 2 * GUARD,), 113, dtype=dtype, device=DEV)
    fr, label = guarded(n, torch.uint8), guarded(n, torch.int32)
    counts, changed, n_roots = guarded(4, torch.int32), guarded(8, torch.int32), guarded(2, torch.int32)
    flags = guarded(L.gs_frontier_flags_bytes(*dims), torch.uint8)
    ws_bytes = L.gs_frontier_workspace_bytes(*dims)
    ws = guarded(ws_bytes, torch.uint8)
    cols = {"root": guarded(K, torch.int32), "size": guarded(K, torch.int32), "faces": guarded(K, torch.int32),
            "sum": guarded(3 * K, torch.int64), "bbox": guarded(6 * K, torch.int32), "best": guarded(2 * K, torch.int32)}
    everything = [fr, label, counts, changed, n_roots, flags, ws] + list(cols.values())

    def inner(t):
        return t[GUARD:]                                    # 16 elements in: 8-byte aligned for every dtype here

    def mark(s=state, d=dims, f=fr, lab=label, c=counts, fl=flags):
        return L.gs_frontier_mark(P(s), None, *d, None if f is None else P(inner(f)), None if lab is None else P(inner(lab)),
                                  None if c is None else P(inner(c)), None if fl is None else P(inner(fl)), stream)

    def relax(d=dims, lab=label, fl=flags, sweep0=0, k=1, ch=changed):
        return L.gs_frontier_relax(*d, None if lab is None else P(inner(lab)), None if fl is None else P(inner(fl)),
                                   sweep0, k, None if ch is None else P(inner(ch)), stream)

    def roots(d=dims, lab=label, w=ws, wb=ws_bytes, nr=n_roots):
        return L.gs_frontier_roots(None if lab is None else P(inner(lab)), *d, None if w is None else P(inner(w)), wb,
                                   None if nr is None else P(inner(nr)), stream)

    def table(rows, capacity, d=dims, s=state, lab=label, w=ws, wb=ws_bytes, skip=None, best_offset=0):
        c = {k: (None if k == skip else P(inner(v)[best_offset if k == "best" else 0:])) for k, v in cols.items()}
        return L.gs_frontier_table(None if s is None else P(s), None if lab is None else P(inner(lab)), None, *d,
                                   None if w is None else P(inner(w)), wb, rows, capacity, c["root"], c["size"],
                                   c["faces"], c["sum"], c["bbox"], c["best"], stream)
    b = frontier.brick()
    assert L.gs_frontier_flags_bytes(0, 1, 1) == 0 and L.gs_frontier_flags_bytes(1, 1025, 1) == 0
    assert L.gs_frontier_workspace_bytes(1, 1, 0) == 0 and L.gs_frontier_workspace_bytes(1025, 1, 1) == 0
    assert L.gs_frontier_flags_bytes(*dims) == 2 * -(-9 // b[0]) * -(-11 // b[1]) * -(-70 // b[2])
    for bad in ((0, 11, 70), (9, 1025, 70), (9, 11, -1)):
        assert mark(d=bad) == INVALID and relax(d=bad) == INVALID and roots(d=bad) == INVALID
        assert table(K, K, d=bad) == INVALID
    assert mark(s=None) == INVALID and mark(f=None) == INVALID and mark(lab=None) == INVALID
    assert mark(c=None) == INVALID and mark(fl=None) == INVALID
    for sweep0, k in ((0, 0), (-1, 1), (0, -2), (0x7fffffff, 1)):
        assert relax(sweep0=sweep0, k=k) == INVALID
    assert relax(lab=None) == INVALID and relax(fl=None) == INVALID and relax(ch=None) == INVALID
    assert roots(lab=None) == INVALID and roots(w=None) == INVALID and roots(nr=None) == INVALID
    assert roots(wb=ws_bytes - 1) == INVALID
    assert table(K, K - 1) == INVALID and table(-1, K) == INVALID and table(1, 0) == INVALID
    assert table(K, K, s=None) == INVALID and table(K, K, lab=None) == INVALID and table(K, K, w=None) == INVALID
    assert table(K, K, wb=ws_bytes - 1) == INVALID and table(K, K, best_offset=1) == INVALID
    for name in cols:
        assert table(K, K, skip=name) == INVALID
    assert L.gs_frontier_brick(None, None, None) == INVALID
    assert b"frontier" in L.gs_last_error()
    torch.cuda.synchronize()
    for t in everything:
        assert (t == 113).all()                             # nothing was launched, nothing was cleared

    # the same buffers through the whole sequence: only the insides change, and a capacity of exactly K holds the table
    assert mark() == 0
    sweeps = 0
    while True:
        assert relax(sweep0=sweeps, k=8) == 0
        quiet = (inner(changed)[:8] == 0).cpu().tolist()
        sweeps += 8
        if True in quiet:
            break
        assert sweeps < 4096
    assert roots() == 0
    assert int(inner(n_roots)[0].item()) == K
    torch.cuda.synchronize()
    for t in cols.values():
        assert (t == 113).all()
    assert table(K, K - 1) == INVALID
    assert table(0, K) == 0                                 # no rows: nothing to do
    torch.cuda.synchronize()
    for t in cols.values():
        assert (t == 113).all()
    assert table(K, K) == 0
    torch.cuda.synchronize()
    for t in everything:
        assert (t[:GUARD] == 113).all() and (t[-GUARD:] == 113).all()
    assert np.array_equal(inner(label)[:n].cpu().numpy().reshape(dims), ref["label"])
    assert np.array_equal(inner(fr)[:n].cpu().numpy().reshape(dims), ref["frontier"])
    assert inner(counts)[:4].cpu().tolist() == ref["counts"].tolist()
    for k in ("root", "size", "faces"):
        assert np.array_equal(inner(cols[k])[:K].cpu().numpy(), ref[k]), k
    assert np.array_equal(inner(cols["sum"])[:3 * K].cpu().numpy().reshape(K, 3), ref["sum"])
    assert np.array_equal(inner(cols["bbox"])[:6 * K].cpu().numpy().reshape(K, 6), ref["bbox"])
    best = inner(cols["best"])[:2 * K].cpu().numpy().reshape(K, 2)
    assert np.array_equal(best[:, 0], ref["best_cell"]) and np.array_equal(best[:, 1], ref["best_cost"])


# ---- end to end on a hand-built volume ------------------------------------------------------------------------------
VOXEL, ROOM, WALL_X, DOOR_Y, DOOR_Z, START = GG.VOXEL, GG.ROOM, GG.WALL_X, GG.DOOR_Y, GG.DOOR_Z, GG.START


@pytest.fixture(scope="module")
def half_seen_room(built_lib):
    """test_geodesic_gpu's room with weight 0 at every x beyond the wall: the far half was never observed."""
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
    vol.weight[WALL_X[1] + 1:] = 0.0
    vol._flags = None
    return vol, vol.esdf()


def test_room_frontier_is_the_door_and_explore_goes_there(half_seen_room):
    vol, field = half_seen_room
    radius = VOXEL
    fc = field.frontiers(robot_radius=radius, start=START)
    state, passable = field.state.cpu().numpy(), field.passable(radius).cpu().numpy()
    assert (state[WALL_X[1] + 1:] == 0).all() and (state[:WALL_X[1] + 1] != 0).all()
    assert fc.start_cell == [8, 6, 30]
    cost = GR.field(passable != 0, [fc.start_cell])
    assert torch.equal(fc.field.cost.cpu(), torch.from_numpy(cost))
    ref = FR.clusters(state, passable, cost)
    assert_clusters(fc, ref)
    cells = np.argwhere(ref["frontier"] != 0)
    print("frontier cells", len(cells), "clusters", fc.n_clusters, "sweeps", fc.sweeps, "sizes", ref["size"].tolist())
    assert len(cells) >= 8 and fc.n_clusters >= 1
    assert (cells[:, 0] <= WALL_X[1]).all()                                  # on the near side
    assert (cells[:, 1] >= DOOR_Y[0]).all() and (cells[:, 1] <= DOOR_Y[1]).all()
    assert (cells[:, 2] >= DOOR_Z[0]).all() and (cells[:, 2] <= DOOR_Z[1]).all()
    assert np.array_equal(fc.centroid.cpu().numpy(), fc.centroid_cells().cpu().numpy() * VOXEL)      # lo = 0
    assert np.array_equal(fc.area_m2.cpu().numpy(), ref["faces"].astype(np.float64) * VOXEL ** 2)
    want_cost = np.where(ref["best_cost"] >= INF, math.inf, ref["best_cost"].astype(np.float64) * VOXEL / 1000.0)
    assert np.array_equal(fc.cost_m.cpu().numpy(), want_cost) and fc.keep.all()

    res = field.explore(START, robot_radius=radius)
    assert res["reachable"] and res["start_cell"] == [8, 6, 30] and res["n_clusters"] == fc.n_clusters
    assert res["n_kept"] == fc.n_clusters and res["n_reachable"] == int((ref["best_cost"] < INF).sum()) >= 1
    row = res["cluster"]
    finite = [i for i in range(len(ref["root"])) if ref["best_cost"][i] < INF]
    assert row == min(finite, key=lambda i: (ref["best_cost"][i], ref["root"][i]))
    got = res["cells"].cpu().numpy()
    goal = tuple(int(v) for v in np.unravel_index(ref["best_cell"][row], ROOM))
    walk, n = GR.path(cost, passable != 0, goal, cost.size)
    assert n == len(got) and np.array_equal(got, walk[::-1])
    assert tuple(got[0]) == (8, 6, 30) and tuple(got[-1]) == goal == tuple(res["goal_cell"])
    assert ref["label"][goal] == ref["root"][row]                            # it ends in a cell of the chosen cluster
    assert res["length_m"] == float(ref["best_cost"][row]) * VOXEL / 1000.0
    assert res["min_clearance_m"] >= radius
    assert res["min_clearance_m"] == float(field.dist.cpu().numpy()[tuple(got.T)].min())
    assert np.array_equal(res["points"].cpu().numpy(), got.astype(np.float64) * VOXEL)
    largest = field.explore(START, robot_radius=radius, order="largest")
    assert largest["reachable"] and largest["cluster"] == min(
        finite, key=lambda i: (-ref["faces"][i], ref["best_cost"][i], ref["root"][i]))

    # min_cells larger than the door's clusters drops them all
    dropped = field.explore(START, robot_radius=radius, min_cells=int(ref["size"].max()) + 1)
    assert dropped["reachable"] is False and dropped["n_kept"] == 0 and dropped["cluster"] is None
    assert dropped["cells"].shape == (0, 3) and dropped["length_m"] == math.inf and dropped["n_clusters"] == fc.n_clusters
    # a robot too wide for the door: no cell of the door lets its centre in, so no kept cluster has a route
    wide = field.explore(START, robot_radius=4 * VOXEL)
    assert wide["reachable"] is False and wide["n_reachable"] == 0 and wide["cluster"] is None
    assert math.isnan(wide["min_clearance_m"])
    assert_clusters(wide["clusters"], FR.clusters(state, field.passable(4 * VOXEL).cpu().numpy(),
                                                 wide["clusters"].field.cost.cpu().numpy()))
    # without a start nothing is priced
    plain = field.frontiers(robot_radius=radius)
    assert plain.field is None and plain.start_cell is None and (plain.best_cost == INF).all()
    assert torch.equal(plain.label, fc.label) and torch.equal(plain.best_cell, plain.root)


def test_frontiers_on_map_finds_the_same_opening(half_seen_room):
    from go_slam_amd import frontier
    vol, field = half_seen_room
    grid = field.occupancy_slice(1, (6 * VOXEL, 8 * VOXEL), robot_radius=VOXEL)
    fm = frontier.frontiers_on_map(grid, (START[0], START[2]))
    cells = grid["cells"].cpu().numpy()
    state = np.where(cells == 254, 1, np.where(cells == 205, 0, 2)).astype(np.uint8)[None]
    free = (cells == 254)[None]
    assert fm.start_cell == (8, 30)
    cost = GR.field(free, [(0, 8, 30)])
    ref = FR.clusters(state, free.astype(np.uint8), cost)
    assert_clusters(fm, ref)
    at = np.argwhere(ref["frontier"][0] != 0)
    print("map frontier cells", at.tolist())
    assert len(at) >= 2 and (at[:, 0] == WALL_X[1]).all()
    assert (at[:, 1] >= DOOR_Z[0]).all() and (at[:, 1] <= DOOR_Z[1]).all()
    assert fm.n_clusters == 1 and (fm.best_cost < INF).all() and fm.keep.all()
    centre = np.array(grid["origin"]) + (fm.centroid_cells().cpu().numpy()[:, 1:] + 0.5) * VOXEL
    assert np.array_equal(fm.centroid.cpu().numpy(), centre)
    assert np.array_equal(fm.length_m.cpu().numpy(), ref["faces"].astype(np.float64) * VOXEL)
    assert np.array_equal(fm.cost_m.cpu().numpy(), ref["best_cost"].astype(np.float64) * VOXEL / 1000.0)
    assert not frontier.frontiers_on_map(grid, min_cells=int(ref["size"][0]) + 1).keep.any()


# ---- whole run ------------------------------------------------------------------------------------------------------
def test_only_tracking_run_ends_with_a_frontier_file(built_lib, tmp_path, monkeypatch):
    from go_slam_amd import frontier, plan
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
                               "esdf": {**esdf_cfg, "frontiers": {"enable": True, "robot_radius": 0.2, "snap": 1.0,
                                                               "min_cells": 2}}})
    stats = returned[0]
    report = frontier.parse_frontiers(open(f"{with_dir}/map/frontiers.txt").read())
    print("map/frontiers.txt:", {k: report[k] for k in frontier.SUMMARY_ORDER})
    assert stats["tsdf_frontier_cells"] == report["n_frontier"] and stats["tsdf_frontier_clusters"] == report["n_clusters"]
    assert stats["tsdf_unknown_fraction"] == report["unknown_fraction"]
    assert stats["tsdf_explore_reachable"] == (report["cluster"] is not None)
    assert report["n_frontier"] >= 1 and 0 < report["unknown_fraction"] < 1
    assert report["n_unknown"] / (report["n_unknown"] + report["n_free"] + report["n_solid"]) == report["unknown_fraction"]
    table = report["clusters"]
    assert len(table["id"]) == report["n_kept"] <= report["n_clusters"] and (table["size"] >= 2).all()
    assert int(np.isfinite(table["cost_m"]).sum()) == report["n_reachable"]
    assert table["size"].sum() <= report["n_frontier"] and (table["faces"] >= table["size"]).all()
    assert np.array_equal(table["area_m2"], table["faces"].astype(np.float64) * 0.1 ** 2)
    extra = [os.path.join("map", "frontiers.txt")]
    if stats["tsdf_explore_reachable"]:
        head, points = plan.parse_path(open(f"{with_dir}/map/explore_path.txt").read())
        row = list(table["id"]).index(report["cluster"])
        assert head["reachable"] and head["length_m"] == table["cost_m"][row] and head["n_points"] == len(points) >= 1
        assert head["min_clearance_m"] >= 0.2
        extra.append(os.path.join("map", "explore_path.txt"))
    EG.TG.whole_run(without_dir, {"enable": True, "source": "sensor", "voxel_size": 0.1, "esdf": esdf_cfg})
    assert not [k for k in returned[1] if "frontier" in k or "explore" in k or "unknown_fraction" in k]
    assert set(returned[0]) - set(returned[1]) == {"tsdf_frontier_cells", "tsdf_frontier_clusters",
                                                   "tsdf_unknown_fraction", "tsdf_explore_reachable"}
    listed = EG.TG.listing(with_dir)
    assert all(p in listed for p in extra)
    assert [p for p in listed if p not in extra] == EG.TG.listing(without_dir)
    assert os.path.exists(f"{with_dir}/map/explore_path.txt") == stats["tsdf_explore_reachable"]
