"""The line-of-sight restatement (tests/sight_restatement.py) judged without a GPU: its walk against an exact rational
slab test, the 26 moves against the geodesic restatement's box rule, the leg lengths, the dynamic programme against a
Dijkstra over the full visibility graph, the properties the definitions promise, the restatement's own 3-D and 2-D cases;
map/path_straight.txt's writer and reader, the refusals that need no device, and the resources of csrc/sight.hip's
kernels."""
import heapq
import itertools
import math
import os
import re
import shutil
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import geodesic_restatement as GR                              # noqa: E402
import sight_restatement as SR                                 # noqa: E402
from go_slam_amd import plan, tsdf                             # noqa: E402

_REF = {}


# ---- the lattices and their paths (tests/test_sight_gpu.py runs the same ones on the device) ----------------------------
def lattice_path(name, passable, seed):
    """(passable, cost, cells int32 [L,3]): the geodesic restatement's field seeded at `seed` and its path down from the
    farthest reachable cell, computed once per name and left unchanged."""
    if name not in _REF:
        cost = GR.field(passable, [seed])
        far = np.unravel_index(np.argmax(np.where(cost < GR.INF, cost, -1)), cost.shape)
        cells, n = GR.path(cost, passable, far, cost.size)
        assert n == len(cells) >= 2
        for a in (passable, cost, cells):
            a.setflags(write=False)
        _REF[name] = (passable, cost, cells)
    return _REF[name]


def random_case():
    """9 x 11 x 70 at 75 % passable, seeded at one end: a path of 75 cells, cost 80336."""
    passable = np.random.default_rng(1).random((9, 11, 70)) < 0.75
    passable[4, 5, 0] = True
    return lattice_path("random", passable, (4, 5, 0))


def two_rooms():
    """[1,24,40]: two rooms split by a wall at columns 19..20 with a door at rows 3..6."""
    passable = np.ones((1, 24, 40), dtype=bool)
    passable[0, :, 19:21] = False
    passable[0, 3:7, 19:21] = True
    return passable


def two_rooms_case():
    """The route from the far corner of the left room's bottom to the right room's bottom: around the door's jambs."""
    passable = two_rooms()
    name = "two rooms"
    if name not in _REF:
        cost = GR.field(passable, [(0, 22, 37)])
        cells, n = GR.path(cost, passable, (0, 21, 2), cost.size)
        for a in (passable, cost, cells):
            a.setflags(write=False)
        _REF[name] = (passable, cost, cells)
    return _REF[name]


def straightened(name, passable, cells, window):
    """The restatement's (index, length), once per (name, window)."""
    key = (name, "straight", window)
    if key not in _REF:
        _REF[key] = SR.straighten(passable, cells, window)
    return _REF[key]


# ---- the walk -------------------------------------------------------------------------------------------------------------
def exact_supercover(d):
    """The cells of the box of 0 and d whose closed unit cube meets the closed segment from 0 to d: per axis the
    parameters t with |t d_k - c_k| <= 1/2, intersected with [0, 1], in exact rationals."""
    box = [range(min(0, v), max(0, v) + 1) for v in d]
    out = set()
    for c in itertools.product(*box):
        lo, hi = Fraction(0), Fraction(1)
        for k in range(3):
            if d[k] == 0:
                if c[k] != 0:                               # |0 - c_k| <= 1/2 only at c_k = 0
                    lo, hi = Fraction(1), Fraction(0)
                continue
            t0, t1 = Fraction(2 * c[k] - 1, 2 * d[k]), Fraction(2 * c[k] + 1, 2 * d[k])
            lo, hi = max(lo, min(t0, t1)), min(hi, max(t0, t1))
        if lo <= hi:
            out.add(c)
    return out


def test_walk_equals_the_exact_supercover():
    sizes = set()
    for d in itertools.product(range(-6, 7), repeat=3):
        cells = SR.walk((0, 0, 0), d)
        assert cells[0] == (0, 0, 0) and cells[-1] == d
        assert len(set(cells)) == len(cells), d             # no cell twice
        assert set(cells) == exact_supercover(d), d
        assert all(min(0, d[k]) <= c[k] <= max(0, d[k]) for c in cells for k in range(3))
        back = SR.walk(d, (0, 0, 0))
        assert set(back) == set(cells) and len(back) == len(cells)          # symmetric
        sizes.add(len(cells) - 1 - sum(abs(v) for v in d))
    assert min(sizes) == 0 < max(sizes)                      # a tie visits more cells than the steps it takes
    shifted = SR.walk((5, 7, 2), (3, 11, 8))                  # translation
    assert shifted == [(c[0] + 5, c[1] + 7, c[2] + 2) for c in SR.walk((0, 0, 0), (-2, 4, 6))]


def test_one_move_is_the_box_rule():
    rng = np.random.default_rng(3)
    outcomes = set()
    for _ in range(40):
        passable = rng.random((3, 3, 3)) < 0.8
        passable[1, 1, 1] = True
        for d in GR.MOVES:
            b = (1 + d[0], 1 + d[1], 1 + d[2])
            box = {(1 + a, 1 + e, 1 + f) for a in {0, d[0]} for e in {0, d[1]} for f in {0, d[2]}}
            assert set(SR.walk((1, 1, 1), b)) == box
            assert SR.sees(passable, (1, 1, 1), b) == GR.allowed(passable, (1, 1, 1), d)
            outcomes.add(SR.sees(passable, (1, 1, 1), b))
    assert outcomes == {True, False}
    corner = np.ones((2, 2, 2), dtype=bool)
    assert not SR.sees(corner, (0, 0, 0), (2, 0, 0)) and not SR.sees(corner, (0, -1, 0), (0, 0, 0))     # an end outside


def test_leg_lengths():
    assert [SR.leg_length((0, 0, 0), d) for d in ((0, 0, 1), (0, -1, 1), (1, -1, 1))] == [1000, 1414, 1732]
    assert sorted(set(SR.leg_length((3, 3, 3), (3 + d[0], 3 + d[1], 3 + d[2])) for d in GR.MOVES)) == [1000, 1414, 1732]
    assert SR.leg_length((0, 0, 0), (1023, 1023, 1023)) == 1771887 == SR.leg_length((1023, 0, 1023), (0, 1023, 0))
    assert SR.leg_length((2, 2, 2), (2, 2, 2)) == 0 and SR.leg_length((0, 0, 0), (3, 4, 0)) == 5000
    for d in ((1, 2, 3), (7, 0, 1), (1000, 1, 0)):
        n = SR.leg_length((0, 0, 0), d)
        assert n * n <= 1000000 * sum(v * v for v in d) < (n + 1) * (n + 1)


def test_segment_min_takes_the_lowest_index_among_equals():
    field = np.full((3, 4, 5), 9, dtype=np.int32)
    assert SR.segment_min(field, (0, 0, 0), (2, 3, 4)) == (9, 0)
    field[1, 1, 2] = field[1, 2, 2] = -4
    assert (1, 1, 2) in SR.walk((0, 0, 0), (2, 3, 4)) and (1, 2, 2) in SR.walk((0, 0, 0), (2, 3, 4))
    assert SR.segment_min(field, (2, 3, 4), (0, 0, 0)) == (-4, (1 * 4 + 1) * 5 + 2)
    assert SR.segment_min(field, (0, 0, 0), (3, 0, 0)) == (-2 ** 31, -1)


# ---- the programme ----------------------------------------------------------------------------------------------------------
def brute_force(passable, cells):
    """The shortest route from the first to the last cell over the complete visibility graph of the path's cells, legs in
    either direction: a heap Dijkstra that knows nothing of windows or of the order of the path."""
    L = len(cells)
    sees = [[i != j and SR.sees(passable, cells[i], cells[j]) for j in range(L)] for i in range(L)]
    dist = [math.inf] * L
    dist[0] = 0
    heap = [(0, 0)]
    while heap:
        d, i = heapq.heappop(heap)
        if d > dist[i]:
            continue
        for j in range(L):
            if sees[i][j] and d + SR.leg_length(cells[i], cells[j]) < dist[j]:
                dist[j] = d + SR.leg_length(cells[i], cells[j])
                heapq.heappush(heap, (dist[j], j))
    return dist[L - 1]


@pytest.mark.parametrize("case", ["random", "two rooms"])
def test_programme_equals_a_dijkstra_over_the_full_visibility_graph(case):
    passable, cost, cells = random_case() if case == "random" else two_rooms_case()
    index, length = straightened(case, passable, cells, len(cells) - 1)
    assert length == brute_force(passable, cells)
    assert index[0] == 0 and index[-1] == len(cells) - 1 and (np.diff(index) > 0).all()
    assert length == sum(SR.leg_length(cells[i], cells[j]) for i, j in zip(index[:-1], index[1:]))


@pytest.mark.parametrize("case", ["random", "two rooms"])
def test_window_one_keeps_every_cell_and_any_window_is_no_longer(case):
    passable, cost, cells = random_case() if case == "random" else two_rooms_case()
    L = len(cells)
    at_start = int(cost[tuple(cells[0])])
    index, length = straightened(case, passable, cells, 1)
    assert index.tolist() == list(range(L)) and length == at_start
    lengths = []
    for window in (1, 2, 4, 16, 63, 64, 65, L - 1, L + 100):
        index, length = straightened(case, passable, cells, window)
        assert index[0] == 0 and index[-1] == L - 1 and length <= at_start
        assert all(0 < j - i <= window and SR.sees(passable, cells[i], cells[j]) for i, j in zip(index[:-1], index[1:]))
        lengths.append(length)
    assert lengths == sorted(lengths, reverse=True) and lengths[-1] == lengths[-2] < lengths[0]


def test_the_optimum_beats_the_greedy_rule_in_3d():
    passable, cost, cells = random_case()
    assert len(cells) == 75 and int(cost[tuple(cells[0])]) == 80336
    index, length = straightened("random", passable, cells, len(cells) - 1)
    g_index, g_length = SR.greedy(passable, cells)
    print("lattice", int(cost[tuple(cells[0])]), "optimum", length, len(index), "greedy", g_length, len(g_index))
    assert (length, len(index)) == (74566, 15) and (g_length, len(g_index)) == (76344, 16)
    assert length < g_length < int(cost[tuple(cells[0])])


def test_two_rooms_larger_windows_give_shorter_routes():
    passable, cost, cells = two_rooms_case()
    L = len(cells)
    assert not SR.sees(passable, cells[0], cells[-1])        # the wall stands between the ends
    door = [i for i, c in enumerate(cells) if 19 <= c[2] <= 20]
    assert door and all(3 <= cells[i][1] <= 6 for i in door)
    lengths = [straightened("two rooms", passable, cells, w)[1] for w in (1, 4, 16, L - 1)]
    print("two rooms: L", L, "lengths", lengths)
    assert lengths[0] == int(cost[tuple(cells[0])]) and lengths[0] > lengths[1] > lengths[2] > lengths[3]
    index, _ = straightened("two rooms", passable, cells, L - 1)
    assert 3 <= len(index) <= 6                              # the ends and the turns at the door


def test_a_blocked_cell_in_the_path():
    passable, cost, cells = random_case()
    L = len(cells)
    blocked = np.array(cells)
    gone = np.argwhere(~passable)[0]
    blocked[L // 2] = gone                                  # a blocked cell in the middle: solved through its neighbours
    index, length = SR.straighten(passable, blocked, L - 1)
    assert index is not None and L // 2 not in index.tolist()
    assert SR.straighten(passable, blocked, 1) == (None, None)
    blocked = np.array(cells)
    blocked[-1] = gone
    assert SR.straighten(passable, blocked, L - 1) == (None, None)
    one = SR.straighten(passable, cells[:1], 256)
    assert one[0].tolist() == [0] and one[1] == 0
    with pytest.raises(ValueError):
        SR.shortcut(np.zeros((3, 1), dtype=np.uint64), cells[:3], 3)


# ---- map/path_straight.txt ----------------------------------------------------------------------------------------------
def test_parse_straight_path_inverts_the_writer_bit_for_bit():
    rng = np.random.default_rng(7)
    pts = rng.standard_normal((5, 3)) * 10.0 ** rng.integers(-6, 6, (5, 3))
    res = {"reachable": True, "straight_length_m": 7.123456789012345, "straight_min_clearance_m": float(np.float32(0.3)),
           "waypoint_points": torch.from_numpy(pts), "length_m": 7.4, "cells": torch.zeros((193, 3), dtype=torch.int32)}
    text = plan.straight_path_text(res)
    assert text.endswith("\n") and len(text.splitlines()) == 2 + len(plan.STRAIGHT_REPORT_ORDER) + 5
    head, back = plan.parse_straight_path(text)
    assert head == {"reachable": True, "length_m": 7.123456789012345, "min_clearance_m": float(np.float32(0.3)),
                    "n_points": 5, "lattice_length_m": 7.4, "n_lattice_points": 193}
    assert back.tobytes() == pts.tobytes()
    nothing = {"reachable": False, "straight_length_m": math.inf, "straight_min_clearance_m": math.nan,
               "waypoint_points": np.zeros((0, 3)), "length_m": math.inf, "cells": np.zeros((0, 3), dtype=np.int32)}
    head, back = plan.parse_straight_path(plan.straight_path_text(nothing))
    assert head["reachable"] is False and head["length_m"] == math.inf and math.isnan(head["min_clearance_m"])
    assert head["n_points"] == 0 and back.shape == (0, 3)
    lattice_text = plan.path_text({"reachable": True, "length_m": 1.0, "min_clearance_m": 0.5, "points": pts})
    for bad in ("", lattice_text, text.replace("lattice_length_m", "lattice_length"), text + "1 2 3\n",
                "\n".join(text.splitlines()[:-1]) + "\n"):
        with pytest.raises(ValueError):
            plan.parse_straight_path(bad)
    with pytest.raises(ValueError):
        plan.parse_path(text)                               # a header of its own


# ---- refusals that need no GPU --------------------------------------------------------------------------------------------
def stub_esdf(dims=(4, 5, 6)):
    state = torch.ones(dims, dtype=torch.uint8)
    return tsdf.ESDF(state, torch.full(dims, 9, dtype=torch.int32), torch.full(dims, 0.3), [0.0, 0.0, 0.0], 0.1, dims, 3)


def test_refusals_before_the_device_is_touched(monkeypatch):
    from go_slam_amd import _lib
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was reached"))
    monkeypatch.setattr(torch.cuda, "current_device", lambda: pytest.fail("the device was reached"))
    ok = torch.ones(2, 3, 4, dtype=torch.uint8)
    cells = torch.zeros(5, 3, dtype=torch.int32)
    for bad in (ok.float(), ok.int(), ok.numpy()):
        with pytest.raises(ValueError, match="passable must be a tensor of uint8"):
            plan.line_of_sight(bad, cells, cells)
        with pytest.raises(ValueError, match="passable must be a tensor of uint8"):
            plan.straighten(bad, cells)
    for bad in (ok, ok.bool(), ok.long(), ok.int().numpy()):
        with pytest.raises(ValueError, match="field must be a tensor of int32"):
            plan.segment_min(bad, cells, cells)
    for bad in (ok[0], torch.ones(1, 1, 1025, dtype=torch.uint8), torch.ones(0, 2, 2, dtype=torch.uint8)):
        with pytest.raises(ValueError, match=r"\[n0,n1,n2\]"):
            plan.line_of_sight(bad, cells, cells)
        with pytest.raises(ValueError, match=r"\[n0,n1,n2\]"):
            plan.segment_min(bad.int(), cells, cells)
        with pytest.raises(ValueError, match=r"\[n0,n1,n2\]"):
            plan.straighten(bad, cells)
    for bad in (cells.float(), cells[:, :2], cells[0], np.zeros((5, 3)), [[0.5, 1, 2]], [[1 << 40, 0, 0]]):
        with pytest.raises(ValueError, match="integers"):
            plan.line_of_sight(ok, bad, cells)
        with pytest.raises(ValueError, match="integers"):
            plan.segment_min(ok.int(), cells, bad)
        with pytest.raises(ValueError, match="integers"):
            plan.straighten(ok, bad)
    with pytest.raises(ValueError, match="a is"):
        plan.line_of_sight(ok, cells, cells[:4])
    with pytest.raises(ValueError, match="at least one cell"):
        plan.straighten(ok, cells[:0])
    for v in (0, -1, 2.0, True, None, "wide"):
        with pytest.raises(ValueError, match="window"):
            plan.straighten(ok, cells, window=v)
    assert plan.straighten_arguments(ok.bool(), [[0, 0, 0], [1, 2, 3]], 7)[0::2] == ((2, 3, 4), 7)

    field = stub_esdf()                                     # a band of 0.3 m
    route = {"cells": cells}
    for robot in (-0.1, 0.31, math.nan):
        with pytest.raises(ValueError, match="robot_radius"):
            field.sees([0.0, 0.0, 0.0], [0.1, 0.1, 0.1], robot_radius=robot)
        with pytest.raises(ValueError, match="robot_radius"):
            field.straighten(route, robot_radius=robot)
    for bad in ([0.0, 0.0], [[0.0, math.nan, 0.0]], [[0.0, math.inf, 0.0]], "here", np.zeros((2, 2, 3))):
        with pytest.raises(ValueError, match="world points"):
            field.sees(bad, [0.0, 0.0, 0.0])
    with pytest.raises(ValueError, match="a_world is"):
        field.sees(np.zeros((2, 3)), np.zeros((3, 3)))
    for v in (0, -3, 1.5, True):
        with pytest.raises(ValueError, match="window"):
            field.straighten(route, window=v)
        with pytest.raises(ValueError, match="window"):
            field.plan([0.0, 0.0, 0.0], [0.1, 0.1, 0.1], straighten=True, window=v)
        with pytest.raises(ValueError, match="window"):
            field.explore([0.0, 0.0, 0.0], straighten=True, window=v)
        with pytest.raises(ValueError, match="window"):
            field.next_view([0.0, 0.0, 0.0], {}, 1, (0.0, 0.2), straighten=True, window=v)
    for bad in (None, [], {"points": cells}):
        with pytest.raises(ValueError, match="route is the dict"):
            field.straighten(bad)
    grid = {"cells": torch.full((4, 6), 254, dtype=torch.uint8), "origin": (0.0, 1.0), "resolution": 0.1}
    with pytest.raises(ValueError, match="window"):
        plan.plan_on_map(grid, (0.05, 1.05), (0.25, 1.25), straighten=True, window=0)


def test_config_values_are_checked(tmp_path):
    assert plan.straighten_config(None) is None and plan.straighten_config(False) is None
    assert plan.straighten_config(True) == plan.DEFAULT_WINDOW == 256
    assert plan.straighten_config({"enable": True}) == 256 and plan.straighten_config({"window": 64}) == 64
    assert plan.straighten_config({"enable": False, "window": 64}) is None
    for bad in (1, "yes", {"enable": 1}, {"window": 0}, {"window": 2.5}, {"window": True}, {"windows": 3}, [True]):
        with pytest.raises(ValueError, match="tsdf.esdf.plan.straighten"):
            plan.straighten_config(bad)

    class Slam:
        output = str(tmp_path)
        cfg = {"tsdf": {"enable": True, "voxel_size": 0.1,
                        "esdf": {"enable": True, "max_distance": 1.0,
                                 "plan": {"enable": True, "straighten": {"enable": True, "window": 0}}}}}

        @property
        def video(self):
            pytest.fail("the keyframes were reached")
    with pytest.raises(ValueError, match="tsdf.esdf.plan.straighten"):
        tsdf.fuse_from_config(Slam(), c2w_list=[])
    Slam.cfg["tsdf"]["esdf"]["plan"]["straighten"] = "on"
    with pytest.raises(ValueError, match="tsdf.esdf.plan.straighten"):
        tsdf.fuse_from_config(Slam(), c2w_list=[])
    assert os.listdir(tmp_path) == []


# ---- the kernels' resources ---------------------------------------------------------------------------------------------
# (VGPRs, static LDS in bytes) the shipped kernels compile to
KERNELS = {"segment_sight_kernel": (22, 0), "segment_min_kernel": (26, 0), "path_sight_kernel": (22, 0),
           "path_shortcut_kernel": (40, 64)}


def test_kernel_resources(tmp_path):
    """test_rooms_cpu.test_kernel_resources for csrc/sight.hip (compile-only: metadata fields of the gfx950 assembly).  No
    kernel uses scratch.  The two walk kernels and the sight matrix take 22 to 26 VGPRs and no LDS, far below the 64 at
    which a SIMD still holds eight waves: their chains of dependent byte loads have eight waves to hide behind.  The
    programme is one workgroup of four waves; its static LDS is the two rows of four 8-byte reduction slots, dp and the
    predecessors are dynamic (6 bytes per path cell)."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "go_slam_amd", "csrc")
    out = tmp_path / "k.s"
    res = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                          "-fno-gpu-rdc", "-munsafe-fp-atomics", "-I", csrc, "-I", os.path.join(ROOT, "include"),
                          "--cuda-device-only", "-S", os.path.join(csrc, "sight.hip"), "-o", str(out)],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-2000:]
    pat = re.compile(r"\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.name:\s+(\S+)\n(?:.*\n)*?"
                     r"\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)")
    seen = {}
    for m in pat.finditer(open(out).read()):
        lds, name, scratch, vgpr = int(m.group(1)), m.group(2), int(m.group(3)), int(m.group(4))
        print(name, "VGPRs", vgpr, "LDS", lds, "scratch", scratch)
        assert scratch == 0, f"{name}: {scratch} B of scratch"
        for key, want in KERNELS.items():
            if key in name:
                seen[key] = seen.get(key, 0) + 1
                assert (vgpr, lds) == want, f"{name}: {vgpr} VGPRs, {lds} B of LDS"
                assert vgpr <= 64                           # eight waves per SIMD
    assert seen == {k: 1 for k in KERNELS}, seen
