"""The scan kernels on the MI355X (csrc/scan.hip, go_slam_amd/scan.py): the cast, the field and the match equal the serial
restatement (tests/scan_restatement.py) with torch.equal into sentinel-filled outputs, the C entries refuse bad arguments
before anything is written, two runs give equal bits, localize_on_map finds the three poses of the recovery scene (also
after save_map / load_map) with the inlier count of the restatement's cast, and an only-tracking run with tsdf.esdf.scan
ends with map/scan_localize.txt."""
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import scan_restatement as R                                   # noqa: E402
import test_esdf_gpu as EG                                     # noqa: E402  (its only-tracking run)
import test_scan_cpu as SC                                     # noqa: E402  (the recovery scene, once)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INVALID = -1
_REF = {}


def gpu(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)  # a copy: the shared references are read-only


def shared(key, make):
    if key not in _REF:
        value = make()
        for a in (value if isinstance(value, tuple) else (value,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _REF[key] = value
    return _REF[key]


MAPS = {"1x1": (1, 1), "1x70": (1, 70), "67x3": (67, 3), "130x129": (130, 129), "scene": (48, 40)}


def base_map(name):
    def make():
        if name == "scene":
            return np.array(SC.scene())
        if name == "1x1":
            return np.full((1, 1), 254, dtype=np.uint8)
        return SC.random_map(MAPS[name], sum(MAPS[name]))      # free, unknown, occupied at probability one third each
    return shared(("map", name), make)


SPECIAL_DIRS = [(1, 0), (0, 1), (-1, 0), (0, -1), (1, 1), (-1, 1), (1, -1), (-1, -1), (0, 0), (32767, 32767), (32767, -1),
                (-1, 32767), (32768, 0), (0, -32768), (-40000, 3), (2, 1), (-32767, 32766)]


def cast_inputs(name, B):
    """(poses [P,2], dirs [P,B,2]): on the border, on an occupied and on an unknown cell where the map has one, outside the
    map on every side, and three drawn ones; per pose the special directions (turned by the pose's number, so that B = 1
    still sees them all), then drawn ones, small and large."""
    def make():
        cells = base_map(name)
        n_u, n_v = cells.shape
        rng = np.random.default_rng(B + n_u)
        poses = [(0, 0), (n_u - 1, n_v - 1), (0, n_v // 2), (n_u // 2, 0), (-1, 0), (n_u, 0), (0, -1), (0, n_v), (n_u // 2, n_v // 2)]
        for value in (0, 205, 254):
            at = np.argwhere(cells == value)
            if len(at):
                poses.append(tuple(at[len(at) // 2]))
        poses += [(int(rng.integers(n_u)), int(rng.integers(n_v))) for _ in range(3)]
        while len(poses) < len(SPECIAL_DIRS):                  # B = 1: one special direction per pose
            poses.append((int(rng.integers(n_u)), int(rng.integers(n_v))))
        P = len(poses)
        dirs = np.zeros((P, B, 2), dtype=np.int32)
        for p in range(P):
            turned = SPECIAL_DIRS[p % len(SPECIAL_DIRS):] + SPECIAL_DIRS[:p % len(SPECIAL_DIRS)]
            row = np.array(turned[:B], dtype=np.int64)
            more = B - len(row)
            if more > 0:
                drawn = np.concatenate([rng.integers(-6, 7, (more // 2, 2)), rng.integers(-32767, 32768, (more - more // 2, 2))])
                row = np.concatenate([row, drawn])
            dirs[p] = row
        return np.array(poses, dtype=np.int32), dirs
    return shared(("cast", name, B), make)


@pytest.mark.parametrize("stop_unknown", [True, False])
@pytest.mark.parametrize("name,B", [("1x1", 1), ("1x1", 64), ("1x70", 63), ("67x3", 64), ("130x129", 257), ("scene", 65),
                                    ("scene", 1)])
def test_cast_equals_the_restatement(built_lib, name, B, stop_unknown):
    from go_slam_amd import scan as S
    cells = base_map(name)
    poses, dirs = cast_inputs(name, B)
    P = len(poses)
    for range2 in (1, 2, cells.shape[0] ** 2 + cells.shape[1] ** 2 + 7):
        want = shared(("cast_ref", name, B, stop_unknown, range2), lambda: R.cast(cells, poses, dirs, range2, stop_unknown))
        out = (torch.full((P, B), 77, dtype=torch.uint8, device=DEV), torch.full((P, B), -7, dtype=torch.int32, device=DEV),
               torch.full((P, B), -7, dtype=torch.int32, device=DEV))
        got = S.cast(gpu(cells), poses, dirs, range2, stop_unknown, out=out)
        for g, o, w, key in zip(got, out, want, ("kind", "hit", "range_mc")):
            assert g is o and torch.equal(g.cpu(), torch.from_numpy(w)), (key, range2)
    if name == "scene":                                        # the walk meets every kind of cell there
        kinds = set(np.unique(want[0]).tolist())
        assert kinds == ({0, 1, 2} if stop_unknown else {0, 1})


def test_cast_without_poses_launches_nothing(built_lib):
    from go_slam_amd import scan as S
    kind, hit, range_mc = S.cast(gpu(base_map("scene")), np.zeros((0, 2), np.int32), np.zeros((0, 5, 2), np.int32), 9)
    assert tuple(kind.shape) == tuple(hit.shape) == tuple(range_mc.shape) == (0, 5)


FIELD_MAPS = {"1x1": (1, 1), "1x130": (1, 130), "130x1": (130, 1), "65x67": (65, 67)}


def field_map(name, content):
    def make():
        shape = FIELD_MAPS[name]
        if content == "drawn":
            cells = SC.random_map(shape, sum(shape))
            cells[np.random.default_rng(3).random(shape) < 0.8] = 254                   # sparse: distances beyond every cap
        elif content == "free":
            cells = np.full(shape, 254, dtype=np.uint8)
        elif content == "occupied":
            cells = np.full(shape, 100, dtype=np.uint8)
        else:                                                   # only unknown beside free: no site
            cells = np.full(shape, 254, dtype=np.uint8)
            cells.reshape(-1)[::3] = 205
        return cells
    return shared(("field_map", name, content), make)


@pytest.mark.parametrize("content", ["drawn", "free", "occupied", "unknown"])
@pytest.mark.parametrize("name", list(FIELD_MAPS))
@pytest.mark.parametrize("radius", [1, 3, 15])
def test_field_equals_the_restatement(built_lib, radius, name, content):
    from go_slam_amd import scan as S
    cells = field_map(name, content)
    want = shared(("field_ref", name, content, radius), lambda: R.field(cells, radius))
    out = torch.full(cells.shape, 250, dtype=torch.uint8, device=DEV)
    got = S.field(gpu(cells), radius, out=(out,))
    assert got is out and torch.equal(got.cpu(), torch.from_numpy(want))
    cap = radius * radius + 1
    if content in ("free", "unknown"):
        assert bool((got == cap).all())
    if content == "occupied":
        assert bool((got == 0).all())


MATCH_SHAPE = (131, 130)
MATCH_WINDOWS = [(0, 0, 131, 130), (5, 7, 1, 1), (0, 0, 3, 4), (0, 126, 3, 4), (128, 0, 3, 4), (128, 126, 3, 4),
                 (10, 3, 2, 63), (10, 3, 2, 64), (10, 66, 2, 64), (10, 0, 2, 65), (130, 0, 1, 130)]


def match_map():
    def make():
        cells = SC.random_map(MATCH_SHAPE, 11)
        cells[np.random.default_rng(12).random(MATCH_SHAPE) < 0.6] = 254
        return cells, R.field(cells, 3)
    return shared("match_map", make)


def match_offsets(Y, B):
    def make():
        rng = np.random.default_rng(Y * 1000 + B)
        off = rng.integers(-140, 141, (Y, B, 2)).astype(np.int64)                        # leaves the map on every side
        special = [(40000, 0), (0, -32769), (-32768, 32767), (32767, 0), (2 ** 31 - 1, -2 ** 31), (0, 0), (32768, 1)]
        for n, value in enumerate(special[:max(B - 1, 0)]):
            off[n % Y, (3 * n + 1) % B] = value
        return off.astype(np.int32)
    return shared(("match_off", Y, B), make)


def signed(word):
    return word - (1 << 64) if word >= (1 << 63) else word


def run_match(S, cost, cells, offsets, window, cap, allow_unknown):
    Y = offsets.shape[0]
    out = (torch.full((Y, window[2], window[3]), 12345, dtype=torch.int32, device=DEV),
           torch.full((1,), 999, dtype=torch.int64, device=DEV))
    got = S.match(gpu(cost), gpu(cells), offsets, window, cap, allow_unknown, out=out)
    assert got[0] is out[0] and got[1] is out[1]
    return got


@pytest.mark.parametrize("allow_unknown", [False, True])
@pytest.mark.parametrize("Y,B", [(1, 1), (3, 64), (1, 65), (3, 300)])
def test_match_equals_the_restatement(built_lib, Y, B, allow_unknown):
    from go_slam_amd import scan as S
    cells, cost = match_map()
    offsets = match_offsets(Y, B)
    for window in MATCH_WINDOWS:
        want = shared(("match_ref", Y, B, allow_unknown, window), lambda: R.match(cost, cells, offsets, window, 10, allow_unknown))
        score, best = run_match(S, cost, cells, offsets, window, 10, allow_unknown)
        assert torch.equal(score.cpu(), torch.from_numpy(want[0].view(np.int32))), window
        assert best.item() == signed(want[1]), window
        again = run_match(S, cost, cells, offsets, window, 10, allow_unknown)
        assert torch.equal(again[0], score) and torch.equal(again[1], best)              # two runs, equal bits


WIDE_SHAPE = (9, 300)
WIDE_WINDOWS = [(0, 0, 9, 300), (2, 10, 3, 255), (2, 10, 3, 256), (2, 40, 3, 257), (8, 44, 1, 256), (0, 299, 9, 1)]


def test_match_windows_across_a_waves_256_cells(built_lib):
    """The kernel gives a lane four consecutive v and a wave 256: windows that end one short of, at and one past that, and
    a map wide enough for a second wave along v."""
    from go_slam_amd import scan as S

    def make():
        cells = SC.random_map(WIDE_SHAPE, 21)
        cells[np.random.default_rng(22).random(WIDE_SHAPE) < 0.6] = 254
        return cells, R.field(cells, 4)
    cells, cost = shared("wide_map", make)
    offsets = shared("wide_off", lambda: np.random.default_rng(23).integers(-12, 13, (2, 65, 2)).astype(np.int32)
                     * np.array([1, 26], dtype=np.int32))                              # along v beyond the map on both sides
    for window in WIDE_WINDOWS:
        want = shared(("wide_ref", window), lambda: R.match(cost, cells, offsets, window, 17, False))
        score, best = run_match(S, cost, cells, offsets, window, 17, False)
        assert torch.equal(score.cpu(), torch.from_numpy(want[0].view(np.int32))), window
        assert best.item() == signed(want[1]), window


def test_match_ties_and_maps_without_a_stand(built_lib):
    from go_slam_amd import scan as S
    room = np.zeros((9, 13), dtype=np.uint8)
    room[1:-1, 1:-1] = 254                                     # an empty rectangular room: half a turn changes nothing
    angles = S.beam_angles(16, 360.0)
    yaws = 2.0 * math.pi * np.arange(4) / 4
    _, _, range_mc = R.cast(room, [[5, 4]], S.beam_directions(angles, yaws[3])[None], 400, True)
    offsets = S.beam_offsets(range_mc[0] / 1000.0, angles, yaws, 1.0)
    cost = R.field(room, 3)
    want = R.match(cost, room, offsets, (0, 0, 9, 13), 10, False)
    score, best = run_match(S, cost, room, offsets, (0, 0, 9, 13), 10, False)
    assert torch.equal(score.cpu(), torch.from_numpy(want[0].view(np.int32))) and best.item() == signed(want[1])
    assert int(score[3, 5, 4]) == int(score[1, 3, 8]) == best.item() >> 32
    assert best.item() & 0xffffffff == (1 * 9 + 3) * 13 + 8     # the mirror image has the lower index and wins
    for value, allow_unknown, stands in ((0, False, False), (205, False, False), (205, True, True)):
        none = np.full((7, 70), value, dtype=np.uint8)
        cost = R.field(none, 2)
        want = R.match(cost, none, offsets, (0, 0, 7, 70), 5, allow_unknown)
        score, best = run_match(S, cost, none, offsets, (0, 0, 7, 70), 5, allow_unknown)
        assert torch.equal(score.cpu(), torch.from_numpy(want[0].view(np.int32))) and best.item() == signed(want[1])
        assert (best.item() == -1) == (not stands) and bool((score == -1).all()) == (not stands)


def test_c_abi_refusals_leave_the_outputs_untouched(built_lib):
    from go_slam_amd import _lib
    L, P = _lib.lib(), _lib.ptr
    stream = _lib.stream_ptr(DEV)
    cells = torch.full((6, 5), 254, dtype=torch.uint8, device=DEV)
    poses = torch.tensor([[1, 1], [2, 3]], dtype=torch.int32, device=DEV)
    dirs = torch.ones((2, 3, 2), dtype=torch.int32, device=DEV)
    kind = torch.full((2, 3), 99, dtype=torch.uint8, device=DEV)
    hit = torch.full((2, 3), -7, dtype=torch.int32, device=DEV)
    rng = torch.full((2, 3), -7, dtype=torch.int32, device=DEV)
    good = dict(cells=P(cells), n_u=6, n_v=5, poses=P(poses), n_poses=2, dirs=P(dirs), n_beams=3, range2=9, stop_unknown=1,
                kind=P(kind), hit=P(hit), range_mc=P(rng))
    bad = [("cells", None), ("poses", None), ("dirs", None), ("kind", None), ("hit", None), ("range_mc", None), ("n_u", 0),
           ("n_u", 1025), ("n_v", 0), ("n_v", 1025), ("n_poses", -1), ("n_poses", 1 << 27), ("n_beams", 0), ("n_beams", 4097),
           ("range2", 0), ("range2", 2 * 1023 * 1023 + 1), ("range2", -4), ("stop_unknown", 2), ("stop_unknown", -1)]
    for key, value in bad:
        assert L.gs_scan_cast(*{**good, key: value}.values(), stream) == INVALID, (key, value)
    assert b"scan_cast" in L.gs_last_error()
    cost = torch.full((6, 5), 77, dtype=torch.uint8, device=DEV)
    good2 = dict(cells=P(cells), n_u=6, n_v=5, R=2, cost=P(cost))
    for key, value in [("cells", None), ("cost", None), ("n_u", 0), ("n_u", 1025), ("n_v", 0), ("n_v", 1025), ("R", 0), ("R", 16),
                       ("R", -1)]:
        assert L.gs_scan_field(*{**good2, key: value}.values(), stream) == INVALID, (key, value)
    assert b"scan_field" in L.gs_last_error()
    field = torch.ones((6, 5), dtype=torch.uint8, device=DEV)
    offsets = torch.zeros((2, 3, 2), dtype=torch.int32, device=DEV)
    score = torch.full((2, 6, 5), 12345, dtype=torch.int32, device=DEV)
    best = torch.full((1,), 999, dtype=torch.int64, device=DEV)
    good3 = dict(cost=P(field), cells=P(cells), n_u=6, n_v=5, offsets=P(offsets), n_yaws=2, n_beams=3, u0=0, v0=0, w_u=6,
                 w_v=5, cap=5, allow_unknown=0, score=P(score), best=P(best))
    bad3 = [("cost", None), ("cells", None), ("offsets", None), ("score", None), ("best", None), ("n_u", 0), ("n_u", 1025),
            ("n_v", 0), ("n_v", 1025), ("n_yaws", 0), ("n_yaws", 1025), ("n_beams", 0), ("n_beams", 4097), ("u0", -1), ("u0", 1),
            ("v0", -1), ("v0", 1), ("w_u", 0), ("w_u", 7), ("w_v", 0), ("w_v", 6), ("w_u", 1 << 31 - 1), ("cap", 0), ("cap", 227),
            ("allow_unknown", 2), ("allow_unknown", -1)]
    for key, value in bad3:
        assert L.gs_scan_match(*{**good3, key: value}.values(), stream) == INVALID, (key, value)
    big = dict(good3, n_u=1024, n_v=1024, w_u=1024, w_v=1024, n_yaws=257)                # 257 * 2^20 candidates > 2^28
    assert L.gs_scan_match(*big.values(), stream) == INVALID
    assert b"scan_match" in L.gs_last_error()
    torch.cuda.synchronize()
    assert bool((kind == 99).all()) and bool((hit == -7).all()) and bool((rng == -7).all()) and bool((cost == 77).all())
    assert bool((score == 12345).all()) and bool((best == 999).all())
    assert L.gs_scan_cast(*good.values(), stream) == 0 and L.gs_scan_field(*good2.values(), stream) == 0
    assert L.gs_scan_match(*good3.values(), stream) == 0
    torch.cuda.synchronize()
    assert bool((kind == 0).all()) and bool((hit == -1).all()) and bool((rng == -1).all())    # an all-free map returns nothing
    assert bool((cost == 5).all()) and bool((score == 3).all()) and best.item() == 3 << 32


def scene_grids(tmp_path):
    from go_slam_amd import tsdf
    grid = {"cells": gpu(SC.scene()), "origin": (0.0, 0.0), "resolution": 1.0}
    tsdf.save_map(str(tmp_path / "map"), grid)
    return grid, tsdf.load_map(str(tmp_path / "map"))


def test_localize_finds_the_scene_poses_also_from_a_saved_map(built_lib, tmp_path):
    from go_slam_amd import scan as S
    cells = SC.scene()
    for grid in scene_grids(tmp_path):
        for (cell, k), (first, _) in zip(SC.SCENE_POSES, SC.SCENE_SCORES):
            yaw = 2.0 * math.pi * k / SC.SCENE_YAWS
            scan = S.scan_on_map(grid, (cell[0] + 0.5, cell[1] + 0.5), yaw, SC.SCENE_BEAMS, 360.0, float(SC.SCENE_RANGE))
            ranges, angles, _ = SC.scene_scan(cell, k)
            assert np.array_equal(scan["angles"], angles) and scan["cells"].tolist() == list(cell)
            assert np.array_equal(scan["ranges_m"].cpu().numpy(), ranges, equal_nan=True)
            assert scan["ranges_m"].device == torch.device(DEV) and scan["kind"].dtype == torch.uint8
            res = S.localize_on_map(grid, scan["ranges_m"], scan["angles"], n_yaw=SC.SCENE_YAWS, max_range=float(SC.SCENE_RANGE))
            print(f"scene pose {cell} yaw {k}:", res)
            assert res["found"] and res["cell"] == cell and res["yaw_index"] == k and res["score"] == first
            assert res["xy"] == (cell[0] + 0.5, cell[1] + 0.5) and res["yaw"] == yaw
            keep = S.valid_beams(ranges, 0.0, float(SC.SCENE_RANGE))
            assert res["n_beams"] == int(keep.sum()) and res["mean_cost"] == first / res["n_beams"]
            kind, _, range_mc = R.cast(cells, [cell], S.beam_directions(angles[keep], yaw)[None],
                                       S.reach2(ranges[keep], 2), True)
            inliers = S.count_inliers(kind[0], range_mc[0], ranges[keep], 2)
            assert res["inliers"] == inliers == res["n_beams"] and res["inlier_fraction"] == 1.0
            near = S.localize_on_map(grid, ranges, angles, n_yaw=SC.SCENE_YAWS, max_range=float(SC.SCENE_RANGE),
                                     around=((cell[0] + 2.5, cell[1] - 1.5), 3.0, yaw + 0.1, 0.5))
            assert near["cell"] == cell and near["yaw_index"] == k and near["score"] == first
    # batched poses: one launch, the same bits as one pose at a time
    xy = np.array([[c[0] + 0.5, c[1] + 0.5] for c, _ in SC.SCENE_POSES])
    yaws = np.array([2.0 * math.pi * k / SC.SCENE_YAWS for _, k in SC.SCENE_POSES])
    both = S.scan_on_map(grid, xy, yaws, SC.SCENE_BEAMS, 360.0, float(SC.SCENE_RANGE))
    assert tuple(both["ranges_m"].shape) == (3, SC.SCENE_BEAMS) and both["cells"].tolist() == [list(c) for c, _ in SC.SCENE_POSES]
    for n, (cell, k) in enumerate(SC.SCENE_POSES):
        assert np.array_equal(both["ranges_m"][n].cpu().numpy(), SC.scene_scan(cell, k)[0], equal_nan=True)
    # a wall the scan does not explain: the score cannot tell, the inlier fraction can
    ranges, angles, _ = SC.scene_scan((10, 8), 5)
    walled = np.array(cells)
    walled[12, 1:20] = 0
    res = S.localize_on_map({"cells": gpu(walled), "origin": (0.0, 0.0), "resolution": 1.0}, ranges, angles,
                            n_yaw=SC.SCENE_YAWS, max_range=float(SC.SCENE_RANGE), around=((10.5, 8.5), 0.0, None, None))
    assert res["found"] and res["cell"] == (10, 8) and 0.0 < res["inlier_fraction"] < 1.0
    # nowhere to stand
    none = S.localize_on_map({"cells": gpu(np.zeros((5, 6), np.uint8)), "origin": (0.0, 0.0), "resolution": 1.0}, ranges, angles, 8)
    assert none["found"] is False and none["n_beams"] == int(np.isfinite(ranges).sum())


def test_match_scan_splits_a_search_beyond_one_launch(built_lib, monkeypatch):
    from go_slam_amd import scan as S
    cell, k = SC.SCENE_POSES[0]
    ranges, angles, yaws = SC.scene_scan(cell, k)
    grid = {"cells": gpu(SC.scene()), "origin": (0.0, 0.0), "resolution": 1.0}
    whole = S.match_scan(grid, ranges, angles, yaws, max_range=float(SC.SCENE_RANGE))
    monkeypatch.setattr(S, "MAX_LANES", 48 * 40 * 5)           # five yaws per launch: seven launches
    split = S.match_scan(grid, ranges, angles, yaws, max_range=float(SC.SCENE_RANGE))
    assert whole["best"] == split["best"] == (k, cell) and whole["best_score"] == split["best_score"] == SC.SCENE_SCORES[0][0]
    assert torch.equal(whole["score"], split["score"]) and tuple(whole["score"].shape) == (SC.SCENE_YAWS, 48, 40)
    cost = S.cost_field(grid, SC.SCENE_R)
    assert torch.equal(cost.cpu(), torch.from_numpy(R.field(SC.scene(), SC.SCENE_R)))


def test_only_tracking_run_ends_with_the_scan_file(built_lib, tmp_path, monkeypatch):
    from go_slam_amd import scan as S
    from go_slam_amd.slam import SLAM
    returned = []
    terminate = SLAM.terminate

    def keeping(self, *args, **kw):
        returned.append(terminate(self, *args, **kw))
        return returned[-1]
    monkeypatch.setattr(SLAM, "terminate", keeping)
    out = str(tmp_path / "with")
    # up along z, a slab just in front of the wall at z = 4, where the cameras see from y = -1.1 down to the floor at
    # y = 1.2: the cameras' columns are free there and the floor is the map's one wall, 12 cells below them
    scan_cfg = {"up_axis": 2, "height": [3.0, 3.6], "beams": 48, "fov_deg": 270.0, "max_range": 3.0, "every": 2, "n_yaw": 24,
                "window_m": 0.5}
    cfg = {"enable": True, "source": "sensor", "voxel_size": 0.1, "esdf": {"enable": True, "max_distance": 1.0, "scan": scan_cfg}}
    EG.TG.whole_run(out, cfg)
    stats = returned[0]
    report = S.parse_scan_localize(open(f"{out}/map/scan_localize.txt").read())
    print("map/scan_localize.txt:", {k: report[k] for k in S.SCAN_SUMMARY_ORDER}, report["rows"][:3])
    assert report["n_yaw"] == 24 and report["poses_tried"] == len(report["rows"])
    n_poses = len(np.load(f"{out}/checkpoints/est_poses.npy"))
    assert report["poses_tried"] + report["poses_skipped"] == len(range(0, n_poses, 2))
    assert 0 <= report["poses_recovered"] <= report["poses_tried"] and report["poses_tried"] >= 1
    assert any(row["found_u"] >= 0 for row in report["rows"])                       # some scan saw the floor
    assert stats["tsdf_scan_poses_tried"] == report["poses_tried"]
    assert stats["tsdf_scan_poses_recovered"] == report["poses_recovered"]
    recovered = 0
    for row in report["rows"]:
        assert 0 <= row["true_yaw_index"] < 24 and 0.0 <= row["inlier_fraction"] <= 1.0
        if row["found_u"] >= 0:
            assert abs(row["found_u"] - row["true_u"]) <= 5 and abs(row["found_v"] - row["true_v"]) <= 5    # window_m / voxel
            turn = abs(row["found_yaw_index"] - row["true_yaw_index"])
            recovered += max(abs(row["found_u"] - row["true_u"]), abs(row["found_v"] - row["true_v"])) <= 1 \
                and min(turn, 24 - turn) <= 1
    assert recovered == report["poses_recovered"]
    assert S.scan_localize_text(report) == open(f"{out}/map/scan_localize.txt").read()
    assert os.path.join("map", "scan_localize.txt") in EG.TG.listing(out)
