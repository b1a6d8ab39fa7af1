"""tests/geodesic_restatement.py against truth that does not come from it -- scipy's Dijkstra on the explicitly built
allowed-move graph, hand-built cases of the corner rule, the line and the cap -- the invariants of its path walk, the
refusals of go_slam_amd.plan and ESDF.passable / plan that need no GPU, the path file's and the map's round trips, and the
compiled kernels' scratch and LDS budgets."""
import math
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import geodesic_restatement as GR                              # noqa: E402
from go_slam_amd import plan, tsdf                             # noqa: E402

INF = GR.INF


def scipy_field(passable, seeds):
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import dijkstra
    n = passable.size
    rows, cols, vals = GR.move_graph(passable)
    graph = csr_matrix((vals, (rows, cols)), shape=(n, n))
    lin = [int(np.ravel_multi_index(tuple(s), passable.shape)) for s in seeds if passable[tuple(s)]]
    if not lin:
        return np.full(passable.shape, INF, dtype=np.int32)
    d = dijkstra(graph, directed=True, indices=lin, min_only=True)
    return np.where(np.isfinite(d), d, INF).astype(np.int32).reshape(passable.shape)


@pytest.mark.parametrize("shape, seeds, seed", [((5, 6, 19), [(2, 3, 4)], 0), ((4, 5, 7), [(0, 0, 0), (3, 4, 6)], 1),
                                                ((1, 17, 18), [(0, 8, 9)], 2), ((1, 9, 30), [(0, 0, 0), (0, 8, 29)], 3)])
def test_restatement_equals_scipy_dijkstra_on_the_move_graph(shape, seeds, seed):
    passable = np.random.default_rng(seed).random(shape) > 0.3
    for s in seeds:
        passable[s] = True
    ref = scipy_field(passable, seeds)
    got = GR.field(passable, seeds)
    assert got.dtype == np.int32 and np.array_equal(got, ref)
    reached = (ref < INF).sum()
    print(shape, "reached", reached, "of", passable.sum(), "passable")
    assert reached > 0.3 * passable.size                    # not vacuous
    assert np.array_equal(GR.move_masks(passable), np.array(
        [[[[GR.allowed(passable, (i, j, k), d) for k in range(shape[2])] for j in range(shape[1])]
          for i in range(shape[0])] for d in GR.MOVES]))


def test_capped_field_is_the_uncapped_one_thresholded():
    passable = np.random.default_rng(0).random((9, 11, 70)) > 0.35
    passable[4, 5, 3] = True
    full = GR.field(passable, [(4, 5, 3)])
    capped = GR.field(passable, [(4, 5, 3)], max_cost=20000)
    assert np.array_equal(capped, np.where(full <= 20000, full, INF))
    assert (full < INF).mean() >= 0.5 and (capped < INF).sum() == 1206


def test_moves_and_weights():
    assert len(GR.MOVES) == 26 and GR.MOVES[0] == (-1, -1, -1) and GR.MOVES[12] == (0, 0, -1) and GR.MOVES[13] == (0, 0, 1)
    assert GR.MOVES[25] == (1, 1, 1)
    assert sorted(set(GR.WEIGHTS)) == [1000, 1414, 1732] and GR.WEIGHTS.count(1000) == 6 and GR.WEIGHTS.count(1732) == 8


def corner_cases():
    """(name, passable, seeds, max_cost, expected cost) of the hand cases; test_geodesic_gpu.py runs them on the GPU."""
    cases = []
    # the 2 x 2 x 2 block with (0,0,1) blocked: from (0,0,0) the diagonals whose box holds (0,0,1) are forbidden -- the
    # face diagonals in the planes d0 = 0 and d1 = 0 and the space diagonal -- and so are those of every other cell
    block = np.ones((2, 2, 2), dtype=bool)
    block[0, 0, 1] = False
    want = np.full((2, 2, 2), INF, dtype=np.int32)
    want[0, 0, 0], want[1, 0, 0], want[0, 1, 0], want[1, 1, 0] = 0, 1000, 1000, 1414
    want[0, 1, 1], want[1, 0, 1], want[1, 1, 1] = 2000, 2000, 2414        # around the blocked cell, never across it
    cases.append(("block", block, [(0, 0, 0)], GR.MAX_COST, want))
    open_block = np.ones((2, 2, 2), dtype=bool)
    want = np.array([[[0, 1000], [1000, 1414]], [[1000, 1414], [1414, 1732]]], dtype=np.int32)
    cases.append(("open block", open_block, [(0, 0, 0)], GR.MAX_COST, want))
    line = np.ones((1, 1, 23), dtype=bool)
    cases.append(("line", line, [(0, 0, 0)], GR.MAX_COST, (1000 * np.arange(23, dtype=np.int32)).reshape(1, 1, 23)))
    want = (1000 * np.arange(23, dtype=np.int32)).reshape(1, 1, 23)
    cases.append(("capped line", line, [(0, 0, 0)], 7000, np.where(want <= 7000, want, INF).astype(np.int32)))
    cases.append(("cap 0", line, [(0, 0, 5)], 0, np.where(np.arange(23) == 5, 0, INF).astype(np.int32).reshape(1, 1, 23)))
    blocked_seed = np.ones((3, 4, 5), dtype=bool)
    blocked_seed[1, 2, 3] = False
    cases.append(("blocked seed", blocked_seed, [(1, 2, 3)], GR.MAX_COST, np.full((3, 4, 5), INF, dtype=np.int32)))
    cases.append(("no seed", blocked_seed, [], GR.MAX_COST, np.full((3, 4, 5), INF, dtype=np.int32)))
    # a 2-D diagonal squeezed between two blocked cells is no passage
    pinch = np.array([[[1, 0], [0, 1]]], dtype=bool)
    cases.append(("pinch", pinch, [(0, 0, 0)], GR.MAX_COST, np.array([[[0, INF], [INF, INF]]], dtype=np.int32)))
    return cases


@pytest.mark.parametrize("case", corner_cases(), ids=lambda c: c[0])
def test_hand_cases(case):
    _, passable, seeds, max_cost, want = case
    assert np.array_equal(GR.field(passable, seeds, max_cost), want)


def test_block_forbids_exactly_the_diagonals_through_the_blocked_cell():
    block = np.ones((2, 2, 2), dtype=bool)
    block[0, 0, 1] = False
    forbidden = {d for d in GR.MOVES if not GR.allowed(block, (0, 0, 0), d)}
    inside = {d for d in GR.MOVES if min(d) >= 0}
    assert forbidden & inside == {(0, 0, 1), (0, 1, 1), (1, 0, 1), (1, 1, 1)}
    assert forbidden - inside == {d for d in GR.MOVES if min(d) < 0}          # those leave the lattice
    for c in np.ndindex(2, 2, 2):                                            # the rule is symmetric in its ends
        for d in GR.MOVES:
            n = tuple(int(a + b) for a, b in zip(c, d))
            if all(0 <= n[i] < 2 for i in range(3)):
                assert GR.allowed(block, c, d) == GR.allowed(block, n, tuple(-v for v in d))


def check_path(cost, passable, cells, start):
    assert tuple(cells[0]) == tuple(start) and cost[tuple(cells[-1])] == 0
    total = 0
    for a, b in zip(cells[:-1], cells[1:]):
        d = tuple(int(v) for v in b - a)
        assert d in GR.MOVES and GR.allowed(passable, tuple(int(v) for v in a), d)
        total += GR.WEIGHTS[GR.MOVES.index(d)]
    assert total == cost[tuple(start)]


def test_path_invariants_and_limits():
    passable = np.random.default_rng(0).random((9, 11, 70)) > 0.35
    passable[4, 5, 3] = True
    cost = GR.field(passable, [(4, 5, 3)])
    far = np.unravel_index(np.argmax(np.where(cost < INF, cost, -1)), cost.shape)
    for start in (far, (4, 5, 3)):
        cells, n = GR.path(cost, passable, start, cost.size)
        assert n == len(cells) >= 1 and n <= cost[start] // 1000 + 1
        check_path(cost, passable, cells, start)
        assert GR.path(cost, passable, start, n)[1] == n
        if n > 1:
            assert GR.path(cost, passable, start, n - 1)[1] == -1
    unreachable = tuple(np.argwhere(cost >= INF)[0])
    assert GR.path(cost, passable, unreachable, 10)[1] == 0 and GR.path(cost, passable, (9, 0, 0), 10)[1] == 0


def test_path_ties_go_to_the_lowest_move_index():
    open_plane = np.ones((1, 3, 3), dtype=bool)
    cost = GR.field(open_plane, [(0, 0, 0), (0, 0, 2)])
    # from (0,1,1) the seeds at d = (0,-1,-1) [move 9] and (0,-1,1) [move 11] both give 1414: move 9 wins
    cells, n = GR.path(cost, open_plane, (0, 1, 1), 5)
    assert n == 2 and cells.tolist() == [[0, 1, 1], [0, 0, 0]]


# ---- refusals that need no GPU --------------------------------------------------------------------------------------
def stub_esdf(dims=(4, 5, 6), radius_voxels=3):
    state = torch.ones(dims, dtype=torch.uint8)
    d2 = torch.full(dims, 4, dtype=torch.int32)
    return tsdf.ESDF(state, d2, torch.full(dims, 0.2), [0.0, 0.0, 0.0], 0.1, dims, radius_voxels)


def test_geodesic_field_refuses_before_the_device_is_touched(monkeypatch):
    from go_slam_amd import _lib
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was reached"))
    ok = torch.ones(2, 3, 4, dtype=torch.uint8)
    with pytest.raises(ValueError, match="uint8 or bool"):
        plan.geodesic_field(ok.float(), [[0, 0, 0]])
    with pytest.raises(ValueError, match="uint8 or bool"):
        plan.geodesic_field(ok.numpy(), [[0, 0, 0]])
    with pytest.raises(ValueError, match=r"\[n0,n1,n2\]"):
        plan.geodesic_field(ok[0], [[0, 0, 0]])
    with pytest.raises(ValueError, match=r"\[n0,n1,n2\]"):
        plan.geodesic_field(torch.ones(1, 1, 1025, dtype=torch.uint8), [[0, 0, 0]])
    with pytest.raises(ValueError, match=r"\[n0,n1,n2\]"):
        plan.geodesic_field(torch.ones(0, 2, 2, dtype=torch.uint8), [])
    for seeds in ([[0, 0]], [[0.5, 0, 0]], [0, 0, 0]):
        with pytest.raises(ValueError, match="seeds must be"):
            plan.geodesic_field(ok, seeds)
    for seeds in ([[2, 0, 0]], [[0, 0, -1]], [[0, 0, 0], [0, 3, 0]]):
        with pytest.raises(ValueError, match="outside the lattice"):
            plan.geodesic_field(ok, seeds)
    for max_cost in (-1, plan.MAX_COST + 1, 1.5, True):
        with pytest.raises(ValueError, match="max_cost"):
            plan.geodesic_field(ok, [[0, 0, 0]], max_cost=max_cost)
    for max_sweeps in (0, -3, 2.0):
        with pytest.raises(ValueError, match="max_sweeps"):
            plan.geodesic_field(ok, [[0, 0, 0]], max_sweeps=max_sweeps)
    assert plan.MAX_COST == 0x3fffffff - 1732


def test_esdf_passable_and_plan_refuse_before_the_device_is_touched(monkeypatch):
    from go_slam_amd import _lib
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was reached"))
    field = stub_esdf()
    for radius in (-0.1, 0.31, math.nan):
        with pytest.raises(ValueError, match="robot_radius"):
            field.passable(radius)
        with pytest.raises(ValueError, match="robot_radius"):
            field.plan([0, 0, 0], [0.1, 0.1, 0.1], robot_radius=radius)
    for point in ([0, 0], [0, 0, math.nan], [0, 0, math.inf], "abc", None):
        with pytest.raises(ValueError, match="three finite"):
            field.plan(point, [0, 0, 0])
        with pytest.raises(ValueError, match="three finite"):
            field.plan([0, 0, 0], point)
    with pytest.raises(ValueError, match="outside the lattice"):
        field.plan([0, 0, 0], [0.36, 0, 0])                 # lattice point 4 of 4
    with pytest.raises(ValueError, match="outside the lattice"):
        field.plan([0, -0.06, 0], [0, 0, 0])
    for snap in (-1.0, math.inf, math.nan):
        with pytest.raises(ValueError, match="snap"):
            field.plan([0, 0, 0], [0.1, 0, 0], snap=snap)
    for max_cost_m in (0.0, -1.0, math.nan, 1e9):
        with pytest.raises(ValueError, match="max_cost_m"):
            field.plan([0, 0, 0], [0.1, 0, 0], max_cost_m=max_cost_m)
    with pytest.raises(ValueError, match=r"\[m,3\]"):
        field.reachable([[0, 0]])
    # the nearest lattice point, and the complement of occupancy_slice's occupied rule (elementwise torch: runs here)
    cells, snap_cells, max_cost = field.plan_arguments([[0.149, 0.151, 0.0], [-0.04, 0.44, 0.54]], 0.1, 0.25, 2.0)
    assert cells == [[1, 2, 0], [0, 4, 5]] and abs(snap_cells - 2.5) < 1e-12 and max_cost == 20000
    field.state[0, 0, 0], field.state[0, 0, 1] = 2, 0
    field.d2[1, 1, 1], field.d2[1, 1, 2] = 3, 4
    p = field.passable(0.2)                                 # floor((0.2 / 0.1)^2) = 4 or 3 in floating point: d2 must exceed it
    occ = int(math.floor((0.2 / 0.1) ** 2))
    assert p.dtype == torch.uint8 and tuple(p.shape) == (4, 5, 6)
    assert p[0, 0, 0] == 0 and p[0, 0, 1] == 0 and p[1, 1, 1] == 0 and p[1, 1, 2] == (1 if 4 > occ else 0)
    assert field.passable(0.1)[0, 0, 1] == 0 and field.passable(0.1, allow_unknown=True)[0, 0, 1] == 1
    assert field.passable(0.1, allow_unknown=True)[0, 0, 0] == 0
    assert int(field.passable(0.0).sum()) == 4 * 5 * 6 - 2


def test_plan_on_map_refuses_before_the_device_is_touched(monkeypatch):
    from go_slam_amd import _lib
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was reached"))
    grid = {"cells": np.full((4, 5), 254, dtype=np.uint8), "origin": (-1.0, 2.0), "resolution": 0.5}
    with pytest.raises(ValueError, match="outside the map"):
        plan.plan_on_map(grid, (-1.01, 2.0), (0.0, 3.0))
    with pytest.raises(ValueError, match="outside the map"):
        plan.plan_on_map(grid, (0.0, 3.0), (1.0, 2.0))       # u = 4 of 4
    with pytest.raises(ValueError, match="goal_xy"):
        plan.plan_on_map(grid, (0.0, 3.0), (0.0,))
    with pytest.raises(ValueError, match="not finite"):
        plan.plan_on_map(grid, (0.0, math.nan), (0.0, 3.0))
    with pytest.raises(ValueError, match="uint8"):
        plan.plan_on_map({**grid, "cells": np.zeros((4, 5), dtype=np.float32)}, (0.0, 3.0), (0.0, 3.0))


def test_plan_on_map_cell_arithmetic_survives_a_map_round_trip(tmp_path, monkeypatch):
    """save_map / load_map give origin and resolution back bit for bit, so a point maps to the same cell before and
    after; the field itself is stubbed by the restatement (this test needs no GPU)."""
    rng = np.random.default_rng(3)
    cells = np.full((7, 9), 254, dtype=np.uint8)
    cells[3, 1:] = 0                                        # a wall with a gap at v = 0
    cells[6, 8] = 205
    grid = {"cells": cells, "origin": (0.1 - 0.5 * 0.07, -0.3 - 0.5 * 0.07), "resolution": 0.07}
    tsdf.save_map(str(tmp_path), grid)
    loaded = tsdf.load_map(str(tmp_path))
    assert loaded["origin"] == grid["origin"] and loaded["resolution"] == grid["resolution"]
    assert np.array_equal(loaded["cells"], cells)

    def host_field(passable, seeds, max_cost=None, max_sweeps=65536):
        dims, seeds, max_cost, _ = plan.field_arguments(passable, seeds, max_cost, max_sweeps)
        p = passable.numpy() != 0
        field = plan.GeodesicField(torch.from_numpy(GR.field(p, seeds, max_cost)), passable.to(torch.uint8), 1)
        field.path = lambda start: torch.from_numpy(GR.path(field.cost.numpy(), p, start, p.size)[0])
        return field
    monkeypatch.setattr(plan, "geodesic_field", host_field)
    for _ in range(8):
        uv = [(int(rng.integers(0, 3)), int(rng.integers(0, 9))), (int(rng.integers(4, 6)), int(rng.integers(0, 9)))]
        xy = [(grid["origin"][0] + (u + rng.uniform(0.01, 0.99)) * 0.07, grid["origin"][1] + (v + rng.uniform(0.01, 0.99)) * 0.07)
              for u, v in uv]
        a, b = plan.plan_on_map(grid, xy[0], xy[1]), plan.plan_on_map(loaded, xy[0], xy[1])
        assert a["start_cell"] == b["start_cell"] == uv[0] and a["goal_cell"] == b["goal_cell"] == uv[1]
        assert a["reachable"] and torch.equal(a["cells"], b["cells"]) and torch.equal(a["points"], b["points"])
        assert a["length_m"] == b["length_m"] and [3, 0] in a["cells"].tolist()           # through the gap
        assert a["cells"][0].tolist() == list(uv[0]) and a["cells"][-1].tolist() == list(uv[1])
        centre = np.array(grid["origin"]) + (a["cells"].numpy().astype(np.float64) + 0.5) * 0.07
        assert np.array_equal(a["points"].numpy(), centre)
    blocked = plan.plan_on_map(grid, (grid["origin"][0] + 0.01, grid["origin"][1] + 0.01),
                               (grid["origin"][0] + 6.5 * 0.07, grid["origin"][1] + 8.5 * 0.07))
    assert not blocked["reachable"] and blocked["length_m"] == math.inf and blocked["cells"].shape[0] == 0
    assert plan.plan_on_map(grid, (grid["origin"][0] + 0.01, grid["origin"][1] + 0.01),
                            (grid["origin"][0] + 6.5 * 0.07, grid["origin"][1] + 8.5 * 0.07), allow_unknown=True)["reachable"]


def test_snap_cell_takes_the_nearest_passable_cell_and_the_lowest_index_on_a_tie():
    passable = torch.zeros(5, 6, 7, dtype=torch.uint8)
    assert plan.snap_cell(passable, [2, 2, 2], 3.0) is None
    passable[2, 2, 4] = passable[2, 4, 2] = passable[4, 2, 2] = passable[0, 2, 2] = 1
    assert plan.snap_cell(passable, [2, 2, 2], 2.0) == [0, 2, 2]             # four at distance 2: the lowest index
    assert plan.snap_cell(passable, [2, 2, 2], 1.9) is None and plan.snap_cell(passable, [2, 2, 2], 0.0) is None
    assert plan.snap_cell(passable, [2, 2, 4], 0.0) == [2, 2, 4]
    passable[3, 3, 2] = 1
    assert plan.snap_cell(passable, [2, 2, 2], 2.0) == [3, 3, 2]             # d2 = 2 beats d2 = 4
    assert plan.snap_cell(passable, [-2, 2, 2], 2.0) == [0, 2, 2] and plan.snap_cell(passable, [-2, 2, 2], 1.5) is None
    assert plan.snap_cell(passable, [9, 9, 9], 2.0) is None


def test_parse_path_inverts_the_writer_bit_for_bit():
    rng = np.random.default_rng(5)
    pts = rng.normal(size=(17, 3)) * np.array([1e-3, 1.0, 1e5])
    res = {"reachable": True, "length_m": float(rng.random()) * 7, "min_clearance_m": float(np.float32(0.1) * 3),
           "points": torch.from_numpy(pts)}
    text = plan.path_text(res)
    head, back = plan.parse_path(text)
    assert head == {"reachable": True, "length_m": res["length_m"], "min_clearance_m": res["min_clearance_m"],
                    "n_points": 17}
    assert back.dtype == np.float64 and np.array_equal(back.view(np.int64), pts.view(np.int64))
    assert len(text.splitlines()) == 2 + 4 + 17 and text.splitlines()[2] == "reachable\tTrue"
    none = {"reachable": False, "length_m": math.inf, "min_clearance_m": math.nan, "points": torch.zeros(0, 3)}
    head, back = plan.parse_path(plan.path_text(none))
    assert head["reachable"] is False and head["length_m"] == math.inf and math.isnan(head["min_clearance_m"])
    assert head["n_points"] == 0 and back.shape == (0, 3)
    with pytest.raises(ValueError):
        plan.parse_path("something else\n")
    with pytest.raises(ValueError):
        plan.parse_path(text + "1.0 2.0 3.0\n")


# ---- compiled resources ---------------------------------------------------------------------------------------------
def test_kernel_resources(tmp_path):
    """tests/test_abi.py's compile-only check for csrc/geodesic.hip: no kernel uses scratch.  LDS budget of the relax
    kernel: the CU has 160 KB, so two workgroups per CU -- the least at which one brick's barrier waits hide behind
    another's rounds -- need at most 80 KB each; under 20 KB, an eighth of the CU, all eight resident workgroups fit (they
    are four waves and a CU holds 32) and LDS never limits occupancy.  The kernel is asked for no more than it took
    before its skeleton moved to csrc/brick_relax.h: the 6172 B of the 4 x 4 x 32 brick's tile, passability and round
    words, and at most 64 VGPRs, eight waves per SIMD."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "go_slam_amd", "csrc")
    out = tmp_path / "k.s"
    res = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                          "-fno-gpu-rdc", "-munsafe-fp-atomics", "-I", csrc, "-I", os.path.join(ROOT, "include"),
                          "--cuda-device-only", "-S", os.path.join(csrc, "geodesic.hip"), "-o", str(out)],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-2000:]
    pat = re.compile(r"\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.name:\s+(\S+)\n(?:.*\n)*?"
                     r"\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)")
    seen = {}
    for m in pat.finditer(open(out).read()):
        lds, name, scratch, vgpr = int(m.group(1)), m.group(2), int(m.group(3)), int(m.group(4))
        print(name, "VGPRs", vgpr, "LDS", lds, "scratch", scratch)
        assert scratch == 0, f"{name}: {scratch} B of scratch"
        for key in ("geodesic_fill_kernel", "geodesic_seed_kernel", "geodesic_relax_kernel", "geodesic_path_kernel"):
            if key in name:
                seen[key] = seen.get(key, 0) + 1
        if "geodesic_relax_kernel" in name:
            assert lds <= 6172 and vgpr <= 64, f"{name}: {lds} B of LDS, {vgpr} VGPRs"
    assert seen == {"geodesic_fill_kernel": 1, "geodesic_seed_kernel": 1, "geodesic_relax_kernel": 1,
                    "geodesic_path_kernel": 1}, seen
