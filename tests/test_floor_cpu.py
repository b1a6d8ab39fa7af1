"""tests/floor_restatement.py against truth that does not come from it, and the Python surface of go_slam_amd/floor.py
without a GPU: the column rule against a search that tries every position of every column, the footprint's free /
occupied split against scipy.ndimage's rank filters under the disc, a hand-built scene whose expected values are written
out here, floor_text / parse_floor, the ValueErrors (before the library is reached) and floor.lift."""
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import floor_restatement as R                                  # noqa: E402
from go_slam_amd import floor as F, tsdf                       # noqa: E402

_REF = {}
VOXEL = 0.05
SCENE_DIMS = (24, 20, 16)
BAND_LOW, BAND_ALL = (1, 7), (1, 12)       # below the table top (k = 9) and with it


def scene_state():
    """24 x 20 x 16 cells, up axis 2, read-only: solid for k <= 1, free 2 .. 13, unseen from 14; a raised floor one cell
    higher for u >= 16; a ramp rising one cell every two columns along v for u in 12 .. 14; a kerb three cells high at
    u = 8, v < 6; a table slab at k = 8 over u in 2 .. 5, v in 12 .. 16; a hole free down to k = 0 at u, v in 10 .. 11; a
    patch of never-seen columns at u in 20 .. 23, v in 0 .. 3."""
    if "scene" not in _REF:
        s = np.zeros(SCENE_DIMS, dtype=np.uint8)
        s[:, :, :2] = 2
        s[:, :, 2:14] = 1
        s[16:, :, 2] = 2
        for v in range(20):
            s[12:15, v, :2 + v // 2] = 2
        s[8, :6, 2:5] = 2
        s[2:6, 12:17, 8] = 2
        s[10:12, 10:12, :14] = 1
        s[20:, :4, :] = 0
        s.setflags(write=False)
        _REF["scene"] = s
    return _REF["scene"]


def search_column(col, p0, p1, H):
    """(position or -1, kind) of one column given as the list of its states by position: every p is tried."""
    n = len(col)
    at = lambda j: col[j] if j < n else 0                      # noqa: E731  beyond the lattice: unseen
    for p in range(p0, p1 + 1):
        if p >= 1 and col[p - 1] == 2 and all(at(j) != 2 for j in range(p, p + H)):
            return p, (1 if all(j < n and col[j] == 1 for j in range(p, p + H)) else 2)
    window = col[max(p0 - 1, 0):min(p1 + H - 1, n - 1) + 1]
    return -1, (0 if 2 not in window and 0 in window else 3)


def random_columns():
    """[15, 20, 12] along the last axis: half of the columns with each state at probability 1/3 per cell, half built from
    runs of 1 .. 6 equal cells (long free runs over solid ones: strict stands with a headroom of 5)."""
    rng = np.random.default_rng(35)
    s = rng.integers(0, 3, (15, 20, 12)).astype(np.uint8)
    for u in range(0, 15, 2):
        for v in range(20):
            col = []
            while len(col) < 12:
                col += [int(rng.choice([2, 1, 1, 0]))] * int(rng.integers(1, 7))
            s[u, v] = col[:12]
    return s


@pytest.mark.parametrize("up_sign", [1, -1])
@pytest.mark.parametrize("H", [1, 3, 5])
def test_column_rule_equals_the_search_over_every_position(H, up_sign):
    base = random_columns()
    kinds = set()
    for case, (p0, p1) in enumerate((a, b) for a in range(12) for b in range(a, 12)):
        up_axis = case % 3                                     # the same columns along another axis of the lattice
        state = np.ascontiguousarray(np.moveaxis(base[:, :, ::up_sign], 2, up_axis))
        floor, kind = R.columns(state, up_axis, up_sign, p0, p1, H)
        assert floor.dtype == np.int16 and kind.dtype == np.uint8 and floor.shape == kind.shape == (15, 20)
        for u in range(15):
            for v in range(20):
                p, want = search_column(base[u, v].tolist(), p0, p1, H)
                k = -1 if p < 0 else (p if up_sign > 0 else 11 - p)
                assert (int(floor[u, v]), int(kind[u, v])) == (k, want), (p0, p1, u, v, base[u, v].tolist())
        kinds |= set(np.unique(kind).tolist())
    assert kinds == {0, 1, 2, 3}


def disc_mask(R2):
    r = int(math.isqrt(R2))
    d = np.arange(-r, r + 1)
    return (d[:, None] ** 2 + d[None, :] ** 2) <= R2


@pytest.mark.parametrize("shape", [(17, 15), (33, 31)])
@pytest.mark.parametrize("R2", [2, 5, 9, 25])
def test_footprint_split_equals_the_rank_filters_under_the_disc(R2, shape):
    from scipy import ndimage
    rng = np.random.default_rng(R2 * 100 + shape[0])
    fp = disc_mask(R2)
    rare = 0.4 / int(fp.sum())                                 # most discs meet neither a blocked column nor a bump
    kind = np.where(rng.random(shape) < rare, 3, 1).astype(np.uint8)
    # plateaus one cell apart with a few bumps, so that every S below separates something
    floor = (2 + (np.arange(shape[0])[:, None] // 6) + (rng.random(shape) < rare) * rng.integers(1, 5, shape)).astype(np.int16)
    floor[kind == 3] = -1
    blocked = kind == 3
    A = ndimage.maximum_filter(blocked.astype(np.int32), footprint=fp, mode="constant", cval=0)
    B = ndimage.maximum_filter(np.where(blocked, -np.inf, floor.astype(np.float64)), footprint=fp, mode="constant",
                               cval=-np.inf)
    C = ndimage.minimum_filter(np.where(blocked, np.inf, floor.astype(np.float64)), footprint=fp, mode="constant",
                               cval=np.inf)
    off_map = ndimage.minimum_filter(np.ones(shape, np.int32), footprint=fp, mode="constant", cval=0) == 0
    seen = set()
    for S in (0, 1, 3):
        cells, why, rough = R.footprint(floor, kind, R2, S)
        with np.errstate(invalid="ignore"):
            ok = (kind == 1) & (A == 0) & (B - floor <= S) & (floor - C <= S)
        assert np.array_equal(cells == R.MAP_FREE, ok & ~off_map)
        assert np.array_equal(cells == R.MAP_UNKNOWN, ok & off_map)
        assert np.array_equal(cells == R.MAP_OCCUPIED, ~ok)
        assert np.array_equal(why != 0, cells == R.MAP_OCCUPIED)
        with np.errstate(invalid="ignore"):
            assert np.array_equal(rough[kind == 1], np.maximum(B - floor, floor - C)[kind == 1].astype(np.int16))
        seen |= set(np.unique(cells).tolist())
    assert seen == {0, 205, 254}


def scene_maps(H, S, band=BAND_LOW, R2=2):
    floor, kind = R.columns(scene_state(), 2, 1, band[0], band[1], H)
    return (floor, kind) + R.footprint(floor, kind, R2, S)


def sides_connected(cells):
    """Whether plan_on_map's passable set (cells == 254) joins (4, 8) on the low floor and (20, 10) on the raised one.
    Its diagonal moves need the whole 2 x 2 box passable, so its components are the 4-connected ones."""
    from scipy import ndimage
    label, _ = ndimage.label(cells == R.MAP_FREE)
    return label[4, 8] != 0 and label[4, 8] == label[20, 10]


def test_hand_built_scene_columns():
    floor, kind, _, _, _ = scene_maps(H=5, S=0)
    want_floor = np.full((24, 20), 2, dtype=np.int16)
    want_kind = np.ones((24, 20), dtype=np.uint8)
    want_floor[16:, :] = 3                                     # the raised floor
    for v in range(20):                                        # the ramp leaves the band [1, 7] at v = 12
        want_floor[12:15, v] = 2 + v // 2 if v < 12 else -1
        want_kind[12:15, v] = 1 if v < 12 else 3
    want_floor[8, :6] = 5                                      # on the kerb
    want_floor[10:12, 10:12], want_kind[10:12, 10:12] = -1, 3  # the hole: seen free to the bottom
    want_floor[20:, :4], want_kind[20:, :4] = -1, 0            # never seen
    assert np.array_equal(floor, want_floor) and np.array_equal(kind, want_kind)      # H = 5: under the table kind 1 at k = 2
    assert (kind[2:6, 12:17] == 1).all() and (floor[2:6, 12:17] == 2).all()
    floor8, kind8, _, _, _ = scene_maps(H=8, S=0)              # H = 8: the slab at k = 8 is in the way, its top beyond the band
    want_floor[2:6, 12:17], want_kind[2:6, 12:17] = -1, 3
    want_kind[12:15, 10:12] = 2                                # the ramp's stand at k = 7 reaches the unseen cell k = 14
    want_kind[10:12, 10:12] = 0                                # and so does the hole's window [0, 14]: nothing solid, one unseen
    assert np.array_equal(floor8, want_floor) and np.array_equal(kind8, want_kind)
    floor14, kind14, _, _, _ = scene_maps(H=14, S=0, band=BAND_ALL)
    want_kind = np.full((24, 20), 2, dtype=np.uint8)           # H = 14 reaches the unseen cells from every stand
    want_kind[10:12, 10:12] = 0                                # the hole: nothing solid, and now unseen cells in the window
    want_kind[20:, :4] = 0
    assert np.array_equal(kind14, want_kind)
    assert (floor14[2:6, 12:17] == 9).all() and (floor14[12:15, 19] == 11).all()      # on the table; the ramp's top


def test_hand_built_scene_footprint_and_connection():
    for S in (0, 1, 2, 3):
        _, _, cells, why, rough = scene_maps(H=5, S=S)
        # the one-cell step between u = 15 and u = 16, away from the ramp and the border
        assert (cells[16, 8], why[16, 8], rough[16, 8]) == ((0, 3, 1) if S == 0 else (254, 0, 1)), S
        assert (cells[17, 8], why[17, 8], rough[17, 8]) == (254, 0, 0)
        # the kerb of three cells blocks itself and its neighbours at every S < 3
        for u in (7, 8, 9):
            assert (cells[u, 1:5] == (0 if S < 3 else 254)).all() and (why[u, 1:5] == (3 if S < 3 else 0)).all(), (S, u)
            assert (rough[u, 1:5] == 3).all()
        assert cells[3, 14] == 254                             # under the table with H = 5
        assert (cells[10, 10], why[10, 10]) == (0, 1) and (cells[9, 9], why[9, 9]) == (0, 2)      # the hole and beside it
        assert (cells[21, 2], why[21, 2]) == (205, 0) and (cells[19, 2], why[19, 2]) == (205, 0)  # unseen and beside it
        assert cells[4, 0] == 205 and cells[0, 8] == 205       # the disc reaches off the map
        assert sides_connected(cells) == (S >= 1), S
    _, _, cells, why, _ = scene_maps(H=8, S=1)                  # the table is too low for H = 8
    assert (cells[2:6, 12:17] == 0).all() and (why[2:6, 12:17] == 1).all()
    assert (cells[1, 14], why[1, 14]) == (0, 2) and cells[3, 10] == 254


def test_floor_text_round_trip_and_summary_on_the_scene():
    floor, kind, cells, why, rough = scene_maps(H=5, S=1)
    grid = {"cells": torch.from_numpy(cells), "why": torch.from_numpy(why), "rough": torch.from_numpy(rough),
            "floor_height": F.floor_heights(torch.from_numpy(floor), -0.3, VOXEL, 1), "resolution": VOXEL}
    report = F.summary(grid)
    assert list(report) == list(F.FLOOR_REPORT_ORDER)
    area = VOXEL * VOXEL
    assert report["drivable_m2"] == int((cells == 254).sum()) * area
    assert report["blocked_m2"] == int((cells == 0).sum()) * area and report["unknown_m2"] == int((cells == 205).sum()) * area
    assert [report[k] for k in ("blocked_no_floor", "blocked_near_no_floor", "blocked_step")] == \
        [int((why == c).sum()) for c in (1, 2, 3)]
    drivable_floor = floor[cells == 254]
    assert report["floor_min_m"] == float(np.float32(-0.3 + (int(drivable_floor.min()) - 0.5) * VOXEL))
    assert report["floor_max_m"] == float(np.float32(-0.3 + (int(drivable_floor.max()) - 0.5) * VOXEL))
    assert report["rough_max_cells"] == 1
    assert F.parse_floor(F.floor_text(report)) == report
    odd = dict(report, drivable_m2=0.1 + 0.2, floor_min_m=math.nan, floor_max_m=-1e-300)
    back = F.parse_floor(F.floor_text(odd))
    assert back["drivable_m2"] == odd["drivable_m2"] and math.isnan(back["floor_min_m"]) and back["floor_max_m"] == -1e-300
    with pytest.raises(ValueError, match="not a map/floor.txt"):
        F.parse_floor("something else\n")
    with pytest.raises(ValueError, match="expected drivable_m2"):
        F.parse_floor(F.floor_text(report).replace("drivable_m2", "drivable"))
    none = dict(grid, cells=torch.zeros_like(grid["cells"]))
    empty = F.summary(none)
    assert empty["drivable_m2"] == 0.0 and math.isnan(empty["floor_min_m"]) and math.isnan(empty["floor_max_m"])
    assert empty["rough_max_cells"] == 0


def test_floor_heights_and_robot_arguments():
    k = torch.tensor([[2, -1], [0, 5]], dtype=torch.int16)
    up = F.floor_heights(k, -0.3, 0.05, 1)
    down = F.floor_heights(k, -0.3, 0.05, -1)
    assert up.dtype == torch.float32 and math.isnan(float(up[0, 1])) and math.isnan(float(down[0, 1]))
    assert float(up[0, 0]) == float(np.float32(-0.3 + 1.5 * 0.05)) and float(down[1, 1]) == float(np.float32(-0.3 + 5.5 * 0.05))
    assert F.robot_arguments(0.05, 0.08, 0.26, 0.06) == (6, 1, 2)          # ceil(5.2), floor(1.2), floor(1.6^2)
    assert F.robot_arguments(0.05, 0.25, 0.05, 0.0) == (1, 0, int(math.floor((0.25 / 0.05) ** 2)))
    assert F.robot_arguments(0.5, 1.0, 1e300, 1e300) == (F.H_MAX, 1024, 4)
    with pytest.raises(ValueError, match=r"smallest usable radius is sqrt\(2\) cells, 0.0707"):
        F.robot_arguments(0.05, 0.07, 0.3, 0.05)                           # floor(1.4^2) = 1
    with pytest.raises(ValueError, match="smallest usable radius"):
        F.robot_arguments(0.05, 32.1 * 0.05, 0.3, 0.05)                    # floor(32.1^2) = 1030
    for bad in (-0.1, math.nan, math.inf, "1", None, True):
        with pytest.raises(ValueError, match="robot_radius"):
            F.robot_arguments(0.05, bad, 0.3, 0.05)
        with pytest.raises(ValueError, match="robot_height"):
            F.robot_arguments(0.05, 0.1, bad, 0.05)
        with pytest.raises(ValueError, match="step_height"):
            F.robot_arguments(0.05, 0.1, 0.3, bad)
    with pytest.raises(ValueError, match="robot_height must be finite and positive"):
        F.robot_arguments(0.05, 0.1, 0.0, 0.05)


def test_refusals_before_the_library_is_reached(monkeypatch):
    from go_slam_amd import _lib
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was reached"))
    state = torch.ones((4, 5, 6), dtype=torch.uint8)
    for bad in (state.int(), state[0], torch.ones((1, 5, 6), dtype=torch.uint8), state.numpy(), None):
        with pytest.raises(ValueError, match="state must be a uint8 tensor"):
            F.columns(bad, 2, 1, 1, 3, 2)
    for axis in (-1, 3, 1.0, True, None):
        with pytest.raises(ValueError, match="up_axis"):
            F.columns(state, axis, 1, 1, 3, 2)
    for sign in (0, 2, -2, 1.0, True, None):
        with pytest.raises(ValueError, match="up_sign"):
            F.columns(state, 2, sign, 1, 3, 2)
    for p0, p1 in ((-1, 3), (3, 2), (0, 6), (6, 6)):
        with pytest.raises(ValueError, match="band"):
            F.columns(state, 2, 1, p0, p1, 2)
    with pytest.raises(ValueError, match="band"):
        F.columns(state, 0, 1, 0, 4, 2)                        # axis 0 has four positions
    for H in (0, -1):
        with pytest.raises(ValueError, match="headroom"):
            F.columns(state, 2, 1, 1, 3, H)
    for H in (1.0, None, True):
        with pytest.raises(ValueError, match="H must be an integer"):
            F.columns(state, 2, 1, 1, 3, H)
    with pytest.raises(ValueError, match="must be on a GPU"):
        F.columns(state, 2, 1, 1, 3, 2)
    floor, kind = torch.zeros((4, 5), dtype=torch.int16), torch.ones((4, 5), dtype=torch.uint8)
    for bad in (floor.int(), floor[0], torch.zeros((1, 5), dtype=torch.int16), None):
        with pytest.raises(ValueError, match="floor must be a int16 tensor"):
            F.footprint(bad, kind, 2, 0)
    for bad in (kind.int(), torch.ones((5, 4), dtype=torch.uint8), None):
        with pytest.raises(ValueError, match="kind must be a uint8 tensor"):
            F.footprint(floor, bad, 2, 0)
    for R2 in (0, 1, 1025, -4):
        with pytest.raises(ValueError, match="R2 must lie"):
            F.footprint(floor, kind, R2, 0)
    with pytest.raises(ValueError, match="S must be >= 0"):
        F.footprint(floor, kind, 2, -1)
    for bad in (2.0, None, True):
        with pytest.raises(ValueError, match="must be an integer"):
            F.footprint(floor, kind, bad, 0)
        with pytest.raises(ValueError, match="must be an integer"):
            F.footprint(floor, kind, 2, bad)
    with pytest.raises(ValueError, match="must be on a GPU"):
        F.footprint(floor, kind, 2, 0)
    # ESDF.floor_map: the band in positions, the robot in cells
    dims = (6, 5, 16)
    field = tsdf.ESDF(torch.ones(dims, dtype=torch.uint8), torch.full(dims, 4, dtype=torch.int32), torch.full(dims, 0.2),
                      [0.0, 0.0, -0.1], VOXEL, dims, 3)
    assert field.floor_arguments(2, (-0.06, 0.26), 0.08, 0.26, 0.06) == (2, 1, 1, 7, 6, 1, 2)
    assert field.floor_arguments(2, (-0.06, 0.26), 0.08, 0.26, 0.06, up_sign=-1) == (2, -1, 8, 14, 6, 1, 2)
    assert field.floor_arguments(0, (-math.inf, math.inf), 0.08, 0.26, 0.0)[:4] == (0, 1, 0, 5)
    with pytest.raises(ValueError, match="no lattice layer"):
        field.floor_map(2, (0.01, 0.03), 0.08, 0.26, 0.06)
    with pytest.raises(ValueError, match="smallest usable radius"):
        field.floor_map(2, (-0.06, 0.26), 0.05, 0.26, 0.06)
    with pytest.raises(ValueError, match="robot_height"):
        field.floor_map(2, (-0.06, 0.26), 0.08, -0.26, 0.06)
    with pytest.raises(ValueError, match="step_height"):
        field.floor_map(2, (-0.06, 0.26), 0.08, 0.26, math.inf)
    with pytest.raises(ValueError, match="up_sign"):
        field.floor_map(2, (-0.06, 0.26), 0.08, 0.26, 0.06, up_sign=0)
    with pytest.raises(ValueError, match="up_axis"):
        field.floor_map(3, (-0.06, 0.26), 0.08, 0.26, 0.06)
    with pytest.raises(ValueError, match="must be on a GPU"):
        field.floor_map(2, (-0.06, 0.26), 0.08, 0.26, 0.06)


def test_floor_config():
    good = {"enable": True, "up_axis": 2, "height": [-0.1, 0.3], "robot_radius": 0.1, "robot_height": 0.3,
            "step_height": 0.05}
    assert F.floor_config(None, 0.05) is None and F.floor_config(dict(good, enable=False), 0.05) is None
    assert F.floor_config({}, 0.05) is None
    assert F.floor_config(good, 0.05) == {"up_axis": 2, "up_sign": 1, "height": (-0.1, 0.3), "robot_radius": 0.1,
                                          "robot_height": 0.3, "step_height": 0.05, "plan": False}
    assert F.floor_config(dict(good, up_sign=-1, plan=True), 0.05)["up_sign"] == -1
    for bad in (True, [], dict(good, speed=1.0), dict(good, enable=1), dict(good, plan="yes"), dict(good, up_axis=3),
                dict(good, up_sign=0), dict(good, height=0.1), dict(good, height=[0.3, -0.1]),
                dict(good, height=[math.nan, 0.1]), dict(good, robot_radius=0.05), dict(good, robot_radius=2.0),
                dict(good, robot_height=0.0), dict(good, step_height=-0.01), dict(good, step_height="low"),
                {k: v for k, v in good.items() if k != "robot_height"}):
        with pytest.raises(ValueError, match="tsdf.esdf.floor"):
            F.floor_config(bad, 0.05)


def test_fuse_from_config_refuses_a_bad_floor_key_before_anything_is_fused(tmp_path):
    import types
    good = {"enable": True, "up_axis": 2, "height": [-0.1, 0.3], "robot_radius": 0.15, "robot_height": 0.3,
            "step_height": 0.05}

    def run(floor_cfg, plan_cfg=None):
        esdf = {"enable": True, "floor": floor_cfg}
        if plan_cfg is not None:
            esdf["plan"] = plan_cfg
        # no video: reaching the fusion would be an AttributeError
        slam = types.SimpleNamespace(cfg={"tsdf": {"enable": True, "voxel_size": 0.1, "bound": [[-1, 1]] * 3, "esdf": esdf}},
                                     output=str(tmp_path))
        return tsdf.fuse_from_config(slam, c2w_list=[])
    with pytest.raises(ValueError, match="smallest usable radius"):
        run(dict(good, robot_radius=0.1))                      # one cell of 0.1 m
    with pytest.raises(ValueError, match="tsdf.esdf.floor: missing"):
        run({"enable": True})
    with pytest.raises(ValueError, match="tsdf.esdf.floor.plan replans the route of tsdf.esdf.plan"):
        run(dict(good, plan=True))
    with pytest.raises(ValueError, match="tsdf.esdf.floor.plan"):
        run(dict(good, plan=True), {"enable": False})
    with pytest.raises(AttributeError):                        # a good key gets as far as the fusion
        run(dict(good, plan=True), {"enable": True})
    with pytest.raises(AttributeError):                        # and a switched-off one is not looked at further
        run({"enable": False, "robot_radius": "wide"})
    assert os.listdir(tmp_path) == []


def test_lift_puts_map_cells_on_the_floor():
    floor, _, cells, _, _ = scene_maps(H=5, S=1)
    for up_axis, up_sign, axes in ((2, 1, (0, 1)), (1, -1, (0, 2))):
        grid = {"cells": torch.from_numpy(cells), "origin": (-1.025, 0.475), "resolution": VOXEL, "axes": axes,
                "up_axis": up_axis, "up_sign": up_sign, "floor_height": F.floor_heights(torch.from_numpy(floor), -0.3, VOXEL, up_sign)}
        route = torch.tensor([[4, 8], [8, 3], [13, 6], [17, 8]], dtype=torch.int32)
        pts = F.lift(grid, route)
        assert pts.dtype == torch.float64 and tuple(pts.shape) == (4, 3)
        for row, (u, v), k in zip(pts.tolist(), route.tolist(), (2, 5, 5, 3)):
            assert row[axes[0]] == -1.025 + (u + 0.5) * VOXEL and row[axes[1]] == 0.475 + (v + 0.5) * VOXEL
            assert row[up_axis] == float(np.float32(-0.3 + (k - 0.5 * up_sign) * VOXEL))
        assert torch.equal(F.lift(grid, route.tolist()), pts)
        assert tuple(F.lift(grid, torch.zeros((0, 2), dtype=torch.int32)).shape) == (0, 3)
        assert tuple(F.lift(grid, []).shape) == (0, 3)
        with pytest.raises(ValueError, match=r"cell 1 of the route, \[10, 10\], has no floor"):
            F.lift(grid, [[4, 8], [10, 10]])
        with pytest.raises(ValueError, match="lies outside the map"):
            F.lift(grid, [[4, 8], [24, 10]])
        with pytest.raises(ValueError, match="lies outside the map"):
            F.lift(grid, [[4, -1]])
        for bad in (torch.zeros((3, 3), dtype=torch.int32), torch.zeros((3, 2)), [[0.5, 1.0]], [1, 2]):
            with pytest.raises(ValueError, match=r"integers \[L,2\]"):
                F.lift(grid, bad)
    with pytest.raises(ValueError, match="dict of ESDF.floor_map"):
        F.lift({"cells": torch.from_numpy(cells)}, [[4, 8]])
