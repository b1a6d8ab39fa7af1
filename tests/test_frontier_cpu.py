"""tests/frontier_restatement.py against truth that does not come from it -- scipy.ndimage's dilation, labelling and
per-label reductions, and hand-built cases -- the refusals of go_slam_amd.frontier and ESDF.frontiers / explore that need
no GPU, ESDF.explore's selection rules on a stub field, the frontier file's round trip, and the compiled kernels' scratch,
register and LDS budgets."""
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

import frontier_restatement as FR                              # noqa: E402
import geodesic_restatement as GR                              # noqa: E402
from go_slam_amd import frontier, plan, tsdf                   # noqa: E402

INF = FR.INF
TABLE = ("root", "size", "faces", "sum", "bbox", "best_cost", "best_cell")


def random_state(shape=(9, 11, 70), seed=0):
    """uint8 states: unknown where r < 0.03, solid where r < 0.53, free otherwise."""
    r = np.random.default_rng(seed).random(shape)
    return np.where(r < 0.03, 0, np.where(r < 0.53, 2, 1)).astype(np.uint8)


def random_open_and_cost(shape, seed=1):
    rng = np.random.default_rng(seed)
    open_ = (rng.random(shape) > 0.2).astype(np.uint8)
    cost = rng.integers(0, 40, size=shape).astype(np.int32) * 500          # many ties
    cost[rng.random(shape) < 0.3] = INF
    return open_, cost


def scipy_truth(state, open_=None, cost=None):
    """The contract through scipy.ndimage and numpy reductions: nothing here comes from the restatement."""
    from scipy import ndimage
    face = ndimage.generate_binary_structure(3, 1)
    near_unknown = ndimage.binary_dilation(state == 0, face, border_value=0)
    fr = (state == 1) & near_unknown
    if open_ is not None:
        fr &= open_ != 0
    comp, K = ndimage.label(fr, structure=np.ones((3, 3, 3)))
    lin = np.arange(state.size, dtype=np.int64).reshape(state.shape)
    ids = np.arange(1, K + 1)
    roots = np.asarray(ndimage.minimum(lin, comp, ids), dtype=np.int64).reshape(K)
    order = np.argsort(roots)                               # rows by ascending root
    rank = np.empty(K, dtype=np.int64)
    rank[order] = np.arange(K)
    label = np.where(comp > 0, np.append(roots, -1)[comp - 1], -1).astype(np.int32)          # comp 0 reads the -1
    row = rank[comp[fr] - 1]
    pad = np.pad(state, 1, constant_values=2)
    n_unknown = sum((pad[tuple(slice(1 + d[a], 1 + d[a] + state.shape[a]) for a in range(3))] == 0).astype(np.int64)
                    for d in FR.FACES)
    coords = np.argwhere(fr)
    out = {"frontier": fr.astype(np.uint8), "label": label,
           "counts": np.array([(state == 0).sum(), (state == 1).sum(), (state == 2).sum(), fr.sum()], dtype=np.uint32),
           "root": roots[order].astype(np.int32), "size": np.bincount(row, minlength=K).astype(np.int32),
           "faces": np.bincount(row, weights=n_unknown[fr], minlength=K).astype(np.int32),
           "sum": np.stack([np.bincount(row, weights=coords[:, a], minlength=K) for a in range(3)], axis=1).astype(np.int64)
           if K else np.zeros((0, 3), dtype=np.int64)}
    boxes = ndimage.find_objects(comp)
    bbox = np.zeros((K, 6), dtype=np.int32)
    for i, sl in enumerate(boxes):
        bbox[rank[i]] = [s.start for s in sl] + [s.stop - 1 for s in sl]
    out["bbox"] = bbox
    c = np.full(state.shape, INF, dtype=np.int64) if cost is None else cost.astype(np.int64)
    key = np.asarray(ndimage.minimum((c << 32) | lin, comp, ids), dtype=np.int64).reshape(K)[order]
    out["best_cost"], out["best_cell"] = (key >> 32).astype(np.int32), (key & 0xffffffff).astype(np.int32)
    return out, comp


def assert_same(got, want, what=""):
    for k in ("frontier", "label", "counts") + TABLE:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (what, k)


@pytest.mark.parametrize("with_masks", [False, True])
def test_restatement_equals_scipy_on_the_random_lattice(with_masks):
    state = random_state()
    open_, cost = random_open_and_cost(state.shape) if with_masks else (None, None)
    want, comp = scipy_truth(state, open_, cost)
    got = FR.clusters(state, open_, cost)
    assert_same(got, want)
    K = len(want["root"])
    if not with_masks:                                      # the case cannot turn vacuous
        assert int(want["counts"][3]) == 524 and K == 64
        assert int((want["size"] == 1).sum()) == 15 and int(want["size"].max()) == 75
        cells = np.argwhere(comp > 0)
        brick = (cells[:, 0] // 4) * 1000000 + (cells[:, 1] // 4) * 1000 + cells[:, 2] // 32
        per = [len(set(brick[comp[tuple(cells.T)] == i + 1])) for i in range(K)]
        assert max(per) == 13 and sum(1 for n in per if n >= 2) == 31
        assert (got["best_cost"] == INF).all() and np.array_equal(got["best_cell"], got["root"])
    else:
        assert K > 40 and (got["best_cost"] < INF).sum() > 20 and (got["best_cost"] == INF).sum() > 0
        assert (got["best_cell"] != got["root"]).sum() > 10


def test_restatement_equals_scipy_on_a_map_shaped_lattice():
    state = random_state((1, 17, 18), seed=4)
    state[0, 3:6, 4:9] = 0
    open_, cost = random_open_and_cost(state.shape, seed=5)
    for o, c in ((None, None), (open_, cost)):
        want, _ = scipy_truth(state, o, c)
        assert_same(FR.clusters(state, o, c), want)
        assert len(want["root"]) >= 3


def cases():
    """(name, state, open, cost, want) of the hand cases, want = {column: expected} with "K" the number of clusters and
    "cells" the frontier cells; test_frontier_gpu.py runs them on the GPU."""
    out = []
    s = np.full((4, 4, 4), 2, dtype=np.uint8)
    s[1, 1, 1] = s[2, 2, 2] = 1
    s[0, 1, 1] = s[3, 2, 2] = 0
    out.append(("corner contact", s, None, None, {"K": 1, "cells": [(1, 1, 1), (2, 2, 2)], "root": [21], "size": [2],
                                                  "faces": [2], "sum": [[3, 3, 3]], "bbox": [[1, 1, 1, 2, 2, 2]]}))
    s = np.full((5, 5, 5), 2, dtype=np.uint8)
    s[1, 1, 1] = s[3, 3, 3] = 1
    s[0, 1, 1] = s[4, 3, 3] = 0
    out.append(("one cell apart", s, None, None, {"K": 2, "cells": [(1, 1, 1), (3, 3, 3)], "root": [31, 93],
                                                  "size": [1, 1], "faces": [1, 1]}))
    out.append(("border is not unknown", np.array([[[1, 1, 2]]], dtype=np.uint8), None, None, {"K": 0, "cells": []}))
    for name, v in (("all unknown", 0), ("all free", 1), ("all solid", 2)):
        counts = [0, 0, 0, 0]
        counts[v] = 60
        out.append((name, np.full((3, 4, 5), v, dtype=np.uint8), None, None, {"K": 0, "cells": [], "counts": counts}))
    s = np.full((3, 3, 3), 2, dtype=np.uint8)
    s[1, 1, 1] = 0
    out.append(("unknown enclosed in solid", s, None, None, {"K": 0, "cells": [], "counts": [1, 0, 26, 0]}))
    s = np.full((2, 2, 2), 2, dtype=np.uint8)
    s[0, 0, 0] = 1
    s[1, 0, 0] = s[0, 1, 0] = s[0, 0, 1] = 0
    out.append(("three unknown faces", s, None, None, {"K": 1, "cells": [(0, 0, 0)], "root": [0], "size": [1],
                                                       "faces": [3], "counts": [3, 1, 4, 1]}))
    strip = np.array([[[0, 0, 0], [1, 1, 1], [2, 2, 2]]], dtype=np.uint8)
    row = [(0, 1, 0), (0, 1, 1), (0, 1, 2)]
    cost = np.full((1, 3, 3), INF, dtype=np.int32)
    cost[0, 1] = [7000, 5000, 5000]
    out.append(("best_cell tie", strip, None, cost, {"K": 1, "cells": row, "root": [3], "size": [3], "faces": [3],
                                                     "best_cost": [5000], "best_cell": [4]}))
    out.append(("no cost", strip, None, None, {"K": 1, "cells": row, "root": [3], "best_cost": [INF], "best_cell": [3]}))
    open_ = np.ones((1, 3, 3), dtype=np.uint8)
    open_[0, 1, 1] = 0
    out.append(("open splits a cluster", strip, open_, cost, {"K": 2, "cells": [(0, 1, 0), (0, 1, 2)], "root": [3, 5],
                                                              "size": [1, 1], "best_cost": [7000, 5000],
                                                              "best_cell": [3, 5]}))
    return out


def check_want(got, want):
    """`got`: {column: numpy array} as FR.clusters gives it."""
    assert len(got["root"]) == want["K"]
    assert [tuple(int(v) for v in c) for c in np.argwhere(got["frontier"] != 0)] == want["cells"]
    assert int(got["counts"][3]) == len(want["cells"]) and int(got["counts"][:3].sum()) == got["frontier"].size
    for k, v in want.items():
        if k not in ("K", "cells"):
            assert np.asarray(got[k]).tolist() == v, k
    for k in TABLE:
        assert len(got[k]) == want["K"]


@pytest.mark.parametrize("case", cases(), ids=lambda c: c[0])
def test_hand_cases(case):
    _, state, open_, cost, want = case
    got = FR.clusters(state, open_, cost)
    check_want(got, want)
    assert_same(got, scipy_truth(state, open_, cost)[0])


# ---- refusals that need no GPU --------------------------------------------------------------------------------------
def stub_esdf(state):
    state = torch.from_numpy(np.ascontiguousarray(state))
    dims = tuple(state.shape)
    return tsdf.ESDF(state, torch.full(dims, 9, dtype=torch.int32), torch.full(dims, 0.3), [0.0, 0.0, 0.0], 0.1, dims, 3)


def test_frontier_clusters_refuses_before_the_device_is_touched(monkeypatch):
    from go_slam_amd import _lib
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was reached"))
    ok = torch.ones(2, 3, 4, dtype=torch.uint8)
    for state in (ok.float(), ok.bool(), ok.numpy()):
        with pytest.raises(ValueError, match="state must be a uint8"):
            frontier.frontier_clusters(state)
    for state in (ok[0], torch.ones(1, 1, 1025, dtype=torch.uint8), torch.ones(0, 2, 2, dtype=torch.uint8)):
        with pytest.raises(ValueError, match=r"\[n0,n1,n2\]"):
            frontier.frontier_clusters(state)
    with pytest.raises(ValueError, match="open must be"):
        frontier.frontier_clusters(ok, open=ok.float())
    with pytest.raises(ValueError, match="open is"):
        frontier.frontier_clusters(ok, open=torch.ones(2, 3, 5, dtype=torch.uint8))
    with pytest.raises(ValueError, match="cost must be"):
        frontier.frontier_clusters(ok, cost=ok.long())
    with pytest.raises(ValueError, match="cost is"):
        frontier.frontier_clusters(ok, cost=torch.zeros(2, 4, 3, dtype=torch.int32))
    for max_sweeps in (0, -3, 2.0, True):
        with pytest.raises(ValueError, match="max_sweeps"):
            frontier.frontier_clusters(ok, max_sweeps=max_sweeps)
    assert frontier.cluster_arguments(ok, ok.bool(), torch.zeros(2, 3, 4, dtype=torch.int32), 7) == ((2, 3, 4), 7)
    assert frontier.INF == 0x3fffffff


def test_esdf_frontiers_and_explore_refuse_before_the_device_is_touched(monkeypatch):
    from go_slam_amd import _lib
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was reached"))
    field = stub_esdf(np.ones((4, 5, 6), dtype=np.uint8))
    for min_cells in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="min_cells"):
            field.frontiers(min_cells=min_cells)
        with pytest.raises(ValueError, match="min_cells"):
            field.explore([0, 0, 0], min_cells=min_cells)
    for order in ("closest", None, 3):
        with pytest.raises(ValueError, match="order"):
            field.explore([0, 0, 0], order=order)
    for radius in (-0.1, 0.31, math.nan):
        with pytest.raises(ValueError, match="robot_radius"):
            field.frontiers(robot_radius=radius)
        with pytest.raises(ValueError, match="robot_radius"):
            field.explore([0, 0, 0], robot_radius=radius)
    for point in ([0, 0], [0, 0, math.nan], "abc"):
        with pytest.raises(ValueError, match="three finite"):
            field.frontiers(start=point)
        with pytest.raises(ValueError, match="three finite"):
            field.explore(point)
    with pytest.raises(ValueError, match="three finite"):
        field.explore(None)
    with pytest.raises(ValueError, match="outside the lattice"):
        field.explore([0.36, 0, 0])
    for snap in (-1.0, math.inf, math.nan):
        with pytest.raises(ValueError, match="snap"):
            field.explore([0, 0, 0], snap=snap)
    for max_cost_m in (0.0, -1.0, math.nan, 1e9):
        with pytest.raises(ValueError, match="max_cost_m"):
            field.frontiers(start=[0, 0, 0], max_cost_m=max_cost_m)


def test_frontiers_on_map_refuses_before_the_device_is_touched(monkeypatch):
    from go_slam_amd import _lib
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was reached"))
    grid = {"cells": np.full((4, 5), 254, dtype=np.uint8), "origin": (-1.0, 2.0), "resolution": 0.5}
    with pytest.raises(ValueError, match="outside the map"):
        frontier.frontiers_on_map(grid, (-1.01, 2.0))
    with pytest.raises(ValueError, match="outside the map"):
        frontier.frontiers_on_map(grid, (1.0, 2.0))          # u = 4 of 4
    with pytest.raises(ValueError, match="start_xy"):
        frontier.frontiers_on_map(grid, (0.0,))
    with pytest.raises(ValueError, match="not finite"):
        frontier.frontiers_on_map(grid, (0.0, math.nan))
    with pytest.raises(ValueError, match="uint8"):
        frontier.frontiers_on_map({**grid, "cells": np.zeros((4, 5), dtype=np.float32)})
    with pytest.raises(ValueError, match="min_cells"):
        frontier.frontiers_on_map(grid, min_cells=0)
    with pytest.raises(ValueError, match="resolution"):
        frontier.frontiers_on_map({**grid, "resolution": 0.0})


# ---- selection -------------------------------------------------------------------------------------------------------
def host_clusters(state, open=None, cost=None, max_sweeps=65536):
    """frontier.frontier_clusters with the restatement in the kernels' place."""
    frontier.cluster_arguments(state, open, cost, max_sweeps)
    got = FR.clusters(state.numpy(), None if open is None else open.numpy(), None if cost is None else cost.numpy())
    table = {k: torch.from_numpy(got[k]) for k in TABLE}
    return frontier.FrontierClusters(torch.from_numpy(got["frontier"]), torch.from_numpy(got["label"]),
                                     torch.from_numpy(got["counts"].astype(np.int64)), table, 1)


def host_field(passable, seeds, max_cost=None, max_sweeps=65536):
    dims, seeds, max_cost, _ = plan.field_arguments(passable, seeds, max_cost, max_sweeps)
    p = passable.numpy() != 0
    field = plan.GeodesicField(torch.from_numpy(GR.field(p, seeds, max_cost)), passable.to(torch.uint8), 1)
    field.path = lambda start: torch.from_numpy(GR.path(field.cost.numpy(), p, tuple(start), p.size)[0])
    return field


def test_choose_applies_the_orders_and_their_ties():
    cost, faces, root, keep = [5000, 3000, 3000, INF, 1000], [4, 9, 9, 50, 2], [2, 7, 11, 13, 17], [1, 1, 1, 1, 0]
    assert frontier.choose(cost, faces, root, keep, "nearest") == 1                  # 3000 twice: the lower root
    assert frontier.choose(cost, faces, root, keep, "largest") == 1                  # 9 faces twice, equal cost: the root
    assert frontier.choose([5000, 3000, 2999, INF, 1000], faces, root, keep, "largest") == 2     # then the cost
    assert frontier.choose(cost, faces, root, [1, 0, 0, 1, 0], "largest") == 0       # the unreachable 50 never wins
    assert frontier.choose(cost, faces, root, [0, 0, 0, 1, 0]) is None
    assert frontier.choose([], [], [], []) is None
    with pytest.raises(ValueError, match="order"):
        frontier.choose(cost, faces, root, keep, "smallest")


def test_explore_selects_routes_and_reports_on_a_stub_field(monkeypatch):
    """A 7 x 12 plane, all free but one unknown cell at the left edge (a cluster of 3 cells around it) and an unknown
    right column (a cluster of 7): the start is nearer to the small one."""
    monkeypatch.setattr(frontier, "frontier_clusters", host_clusters)
    monkeypatch.setattr(plan, "geodesic_field", host_field)
    state = np.ones((1, 7, 12), dtype=np.uint8)
    state[0, 3, 0] = 0
    state[0, :, 11] = 0
    field = stub_esdf(state)
    start = [0.0, 0.3, 0.3]
    fc = field.frontiers(start=start)
    assert fc.n_clusters == 2 and fc.root.tolist() == [10, 24] and fc.size.tolist() == [7, 3]
    assert fc.best_cost.tolist() == [7000, 2000] and fc.best_cell.tolist() == [3 * 12 + 10, 3 * 12 + 1]
    assert fc.start_cell == [0, 3, 3] and fc.keep.tolist() == [True, True]
    assert fc.cost_m.tolist() == [7000 * 0.1 / 1000.0, 2000 * 0.1 / 1000.0]
    assert fc.area_m2.tolist() == [7 * 0.1 ** 2, 3 * 0.1 ** 2]
    assert np.array_equal(fc.centroid.numpy(), fc.centroid_cells().numpy() * 0.1)
    assert fc.centroid_cells().tolist() == [[0.0, 3.0, 10.0], [0.0, 3.0, 1 / 3]]
    near = field.explore(start)
    assert near["reachable"] and near["cluster"] == 1 and near["goal_cell"] == [0, 3, 1]
    assert near["cells"].tolist() == [[0, 3, 3], [0, 3, 2], [0, 3, 1]] and near["length_m"] == 2000 * 0.1 / 1000.0
    assert near["n_clusters"] == 2 and near["n_kept"] == 2 and near["n_reachable"] == 2
    assert near["start_cell"] == [0, 3, 3] and abs(near["min_clearance_m"] - 0.3) < 1e-6
    assert np.array_equal(near["points"].numpy(), near["cells"].numpy().astype(np.float64) * 0.1)
    big = field.explore(start, order="largest")
    assert big["cluster"] == 0 and big["goal_cell"] == [0, 3, 10] and big["cells"].shape[0] == 8
    assert big["cells"][0].tolist() == [0, 3, 3] and big["cells"][-1].tolist() == [0, 3, 10]
    kept = field.explore(start, min_cells=4)
    assert kept["cluster"] == 0 and kept["n_kept"] == 1 and kept["n_reachable"] == 1
    none = field.explore(start, min_cells=8)
    assert none["reachable"] is False and none["cluster"] is None and none["cells"].shape == (0, 3)
    assert none["length_m"] == math.inf and math.isnan(none["min_clearance_m"]) and none["n_kept"] == 0
    capped = field.explore(start, max_cost_m=0.25)           # 2500 milli-voxels: only the near cluster has a route
    assert capped["cluster"] == 1 and capped["n_reachable"] == 1 and capped["n_kept"] == 2
    assert field.explore(start, order="largest", max_cost_m=0.25)["cluster"] == 1
    state[0, :, 2] = 2                                       # a wall between the start and the near cluster
    state[0, :, 9] = 2
    walled = stub_esdf(state).explore(start)
    assert walled["reachable"] is False and walled["n_clusters"] == 2 and walled["n_reachable"] == 0
    # the text of such a result
    report = frontier.summary(fc, near["cluster"])
    assert report["n_frontier"] == 10 and report["n_unknown"] == 8 and report["unknown_fraction"] == 8 / 84
    assert report["cluster"] == 1 and report["clusters"]["id"].tolist() == [0, 1]
    back = frontier.parse_frontiers(frontier.frontiers_text(report))
    assert back["clusters"]["cost_m"].tolist() == fc.cost_m.tolist()


def same_report(a, b):
    assert list(a) == list(b)
    for k in frontier.SUMMARY_ORDER:
        assert a[k] == b[k] and type(a[k]) is type(b[k]), k
    for c in frontier.CLUSTER_COLUMNS:
        x, y = np.asarray(a["clusters"][c]), np.asarray(b["clusters"][c])
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), c


def test_parse_frontiers_inverts_the_writer_bit_for_bit():
    rng = np.random.default_rng(7)
    n = 9
    table = {"id": np.arange(n, dtype=np.int64) * 2, "root": rng.integers(0, 1 << 30, n).astype(np.int64),
             "size": rng.integers(1, 1000, n).astype(np.int64), "faces": rng.integers(1, 3000, n).astype(np.int64),
             "area_m2": rng.random(n) * 1e-3, "centroid_x": rng.normal(size=n) * 1e5, "centroid_y": rng.normal(size=n),
             "centroid_z": rng.normal(size=n) * 1e-4, "cost_m": rng.random(n) * 30}
    table["cost_m"][[2, 5]] = math.inf
    report = {"n_unknown": 123456, "n_free": 77, "n_solid": 9, "n_frontier": 4321, "unknown_fraction": 123456 / 123542,
              "n_clusters": 20, "n_kept": n, "n_reachable": 7, "cluster": 4, "clusters": table}
    text = frontier.frontiers_text(report)
    same_report(frontier.parse_frontiers(text), report)
    lines = text.splitlines()
    assert len(lines) == 2 + len(frontier.SUMMARY_ORDER) + n and lines[2] == "n_unknown\t123456"
    empty = {**report, "n_clusters": 0, "n_kept": 0, "n_reachable": 0, "cluster": None,
             "clusters": {c: np.zeros(0, dtype=np.int64 if c in ("id", "root", "size", "faces") else np.float64)
                          for c in frontier.CLUSTER_COLUMNS}}
    back = frontier.parse_frontiers(frontier.frontiers_text(empty))
    same_report(back, empty)
    assert back["cluster"] is None
    with pytest.raises(ValueError):
        frontier.parse_frontiers("something else\n")
    with pytest.raises(ValueError):
        frontier.parse_frontiers(text + lines[-1] + "\n")


# ---- compiled resources ---------------------------------------------------------------------------------------------
KERNELS = ("frontier_mark_kernel", "frontier_relax_kernel", "frontier_count_kernel", "frontier_scan_kernel",
           "frontier_emit_kernel", "frontier_table_kernel")


def test_kernel_resources(tmp_path):
    """test_geodesic_cpu.test_kernel_resources for csrc/frontier.hip, by the reasoning stated there: no kernel uses
    scratch, and the relax kernel takes no more than before its skeleton moved to csrc/brick_relax.h: the 4940 B of the
    4 x 4 x 32 brick's tile of labels and round words, far below the 20 KB at which LDS would limit occupancy, and at
    most 64 VGPRs, eight waves per SIMD."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "go_slam_amd", "csrc")
    out = tmp_path / "k.s"
    res = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                          "-fno-gpu-rdc", "-munsafe-fp-atomics", "-I", csrc, "-I", os.path.join(ROOT, "include"),
                          "--cuda-device-only", "-S", os.path.join(csrc, "frontier.hip"), "-o", str(out)],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-2000:]
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
        if "frontier_relax_kernel" in name:
            assert lds <= 4940 and vgpr <= 64, f"{name}: {lds} B of LDS, {vgpr} VGPRs"
    assert seen == {k: 1 for k in KERNELS}, seen
