"""Objects without a GPU (go_slam_amd/tsdf_objects.py over tests/tsdf_objects_restatement.py): every branch of the mark rule
on single cells, the restated labels against scipy.ndimage, the table against a direct computation, the policy for
structure planes, the host steps (axes from exact moments, the sign rule, another frame, the text round trip, refusals
before the library is reached), and the restated pipeline on an analytic room -- a floor, a wall, two boxes standing on the
floor (one turned by 30 degrees) and a floating ball -- straight and in a world tilted by 20 degrees of roll and 10 of
pitch: exactly three objects, each where, as large and turned as the geometry says."""
import math
import os
import sys
import types

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from go_slam_amd import tsdf_objects as TO                     # noqa: E402
from go_slam_amd import tsdf_planes as TP                      # noqa: E402
import test_tsdf_planes_cpu as PC                              # noqa: E402  (the lattice, tilt, one_cell)
import tsdf_align_restatement as AR                            # noqa: E402
import tsdf_merge_restatement as MR                            # noqa: E402
import tsdf_objects_restatement as OR                          # noqa: E402
import tsdf_planes_restatement as PR                           # noqa: E402

F = np.float32
VOXEL, DIMS, LO, CHUNK = PC.VOXEL, PC.DIMS, PC.LO, PC.CHUNK
TRUNC = 3 * VOXEL
COS2 = float(np.float32(math.cos(math.radians(10.0)) ** 2))
UP_D = np.array([0.0, -1.0, 0.0])                              # y grows downward
TURN_B = AR.rotation([0.0, math.radians(30.0), 0.0])           # box B, about up
# name: centre, size along (x, y, z) of its own frame, rotation of that frame, size along (up, long, short), long axis
THINGS = {"box_a": (np.array([0.0, 0.8, 1.0]), np.array([0.8, 0.8, 0.6]), np.eye(3), (0.8, 0.8, 0.6), np.array([1.0, 0, 0])),
          "box_b": (np.array([1.6, 0.7, 2.5]), np.array([1.2, 1.0, 0.5]), TURN_B, (1.0, 1.2, 0.5), TURN_B @ [1.0, 0, 0]),
          "ball": (np.array([0.3, 0.2, 3.0]), 0.35, None, (0.7, 0.7, 0.7), None)}


# ---- the analytic room ----------------------------------------------------------------------------------------------------
def room_distance(x):
    """The signed distance (positive in free space) of the points x float64 [...,3] of the scene's own world to the nearest
    of the floor y = 1.2, the wall z = 4, the two boxes and the ball."""
    d = np.minimum(1.2 - x[..., 1], 4.0 - x[..., 2])
    for centre, size, R, _, _ in THINGS.values():
        if R is None:
            d = np.minimum(d, np.linalg.norm(x - centre, axis=-1) - size)
            continue
        q = np.abs((x - centre) @ R) - 0.5 * size               # the point in the box's frame
        d = np.minimum(d, np.linalg.norm(np.maximum(q, 0.0), axis=-1) + np.minimum(q.max(-1), 0.0))
    return d


def room(M=None):
    """The room as a restated volume on the plane tests' lattice, in the world x_S = M x_D (None: the scene's own)."""
    ax = [LO[a] + VOXEL * np.arange(DIMS[a], dtype=np.float64) for a in range(3)]
    P = np.stack(np.meshgrid(*ax, indexing="ij"), -1)
    if M is not None:
        P = (P - M[:3, 3]) @ M[:3, :3]                           # M^-1 x
    return MR.volume(np.clip(room_distance(P) / TRUNC, -1.0, 1.0), np.ones(DIMS), LO, VOXEL, TRUNC)


_WORLDS = {}


def world(name):
    """{"M", "vol", "planes", "floor", "structure", "index", "up", "objects"} of the "straight" or the "tilted" room: the
    restated planes, the floor under the world's up, the structure planes and the restated objects.  Computed once."""
    if name not in _WORLDS:
        M = np.eye(4) if name == "straight" else PC.tilt()
        vol = room(None if name == "straight" else M)
        planes = PR.find_planes(vol, CHUNK)
        up = M[:3, :3] @ UP_D
        floor = TP.floor_plane(planes, up)
        structure, index = TO.structure_planes(planes, floor)
        _WORLDS[name] = {"M": M, "vol": vol, "planes": planes, "floor": floor, "structure": structure, "index": index,
                         "up": up, "objects": OR.find_objects(vol, structure)}
    return _WORLDS[name]


def match(boxes, M):
    """{name: the box whose centre is nearest the thing's}."""
    out = {}
    for name, (centre, *_rest) in THINGS.items():
        c = M[:3, :3] @ centre + M[:3, 3]
        out[name] = min(boxes, key=lambda b: float(np.linalg.norm(b["centre"] - c)))
    return out


# Two voxels, one per side (the sample point of a cell at a convex edge can lie up to a voxel outside the edge), would be
# 0.25 m.  The restatement's worst extent, box A's short side in the tilted world, is 0.8537 m against 0.6: 0.2537 m, of which
# 0.024 m is the 0.8 m side seen along a long axis that the cells' moments put 1.69 degrees off (0.8 sin 1.69).  The bound
# is that measured value plus 10 %.
EXTENT_BOUND = 1.1 * 0.25368347


def check_boxes(boxes, w, extent_bound=EXTENT_BOUND):
    """The bounds from the geometry: centres within a voxel, extents within EXTENT_BOUND, box B's long axis within
    atan(voxel / 1.2 m) of 30 degrees modulo a half turn, the boxes on the floor alone, the ball on nothing."""
    M = w["M"]
    assert len(boxes) == 3
    found = match(boxes, M)
    assert len({id(b) for b in found.values()}) == 3
    worst_c = worst_e = 0.0
    for name, (centre, _size, _R, extent, long) in THINGS.items():
        b = found[name]
        c = M[:3, :3] @ centre + M[:3, 3]
        worst_c = max(worst_c, float(np.linalg.norm(b["centre"] - c)))
        got = sorted(b["size_m"][1:], reverse=True) if name == "ball" else list(b["size_m"][1:])
        err = np.abs(np.array([b["size_m"][0], *got]) - extent)
        worst_e = max(worst_e, float(err.max()))
        print(f"{name}: {b['cells']} cells, centre off {np.linalg.norm(b['centre'] - c):.4f} m, size "
              f"{np.round(b['size_m'], 3).tolist()} against {extent}, elongation {b['elongation']:.3f}, touches {b['touches']}, "
              f"above {b['above_m']}")
        assert np.linalg.norm(b["centre"] - c) <= VOXEL, name
        assert err.max() <= extent_bound, (name, err)
        assert np.abs(b["axes"] @ b["axes"].T - np.eye(3)).max() < 1e-12 and np.linalg.det(b["axes"]) > 0
        assert b["touches"] == ([] if name == "ball" else [0]), name      # structure plane 0 is the floor
        assert len(b["touches"]) < 2
        if name == "ball":
            assert b["above_m"][0] > 0.5                        # it floats: 0.65 m above the floor
        else:
            assert abs(b["above_m"][0]) <= VOXEL and abs(b["above_m"][1] - extent[0]) <= VOXEL
        if name == "box_b":
            cosang = abs(float(b["axes"][1] @ (M[:3, :3] @ long)))
            ang = math.degrees(math.acos(min(1.0, cosang)))
            print(f"box_b: long axis {ang:.3f} degrees off, bound {math.degrees(math.atan(VOXEL / 1.2)):.3f}")
            assert ang <= math.degrees(math.atan(VOXEL / 1.2))
    print(f"worst centre error {worst_c:.4f} m (bound {VOXEL}), worst extent error {worst_e:.4f} m (bound {extent_bound})")


# ---- the mark rule, cell by cell --------------------------------------------------------------------------------------------
I, J, K = np.meshgrid([0, 1], [0, 1], [0, 1], indexing="ij")
GOOD = 0.25 * (I + J - 1)                                       # g = (0.25, 0.25, 0), f = 0, p = (0.5, 0.5, 0.5)
DIAG = np.array([1.0, 1.0, 0.0]) / math.sqrt(2.0)
ON = [*DIAG, float(DIAG @ [0.5, 0.5, 0.5])]                     # through p, along g
FAR = [*DIAG, 5.0]
ACROSS = [0.0, 0.0, 1.0, 0.5]                                   # through p, square to g: near, never agreeing
ACROSS2 = [0.0, 0.0, -1.0, -0.5]


def mark_one(values, planes, band=0.25, weights=None, **kw):
    m = OR.mark(PC.one_cell(values, weights), np.array(planes, np.float64).reshape(-1, 4), COS2, band, **kw)
    return int(m["kind"][0, 0, 0]), int(m["label"][0, 0, 0]), m["counts"].tolist()


def test_every_branch_of_the_mark_rule_on_one_cell():
    assert mark_one(GOOD, []) == (1, 0, [1, 1, 0, 0])                        # no planes: every sample is an object cell
    assert mark_one(GOOD, [FAR]) == (1, 0, [1, 1, 0, 0])                     # far from the plane
    assert mark_one(GOOD, [ON]) == (2, -1, [1, 0, 1, 0])                     # on it
    assert mark_one(GOOD, [[*(-DIAG), -ON[3]]]) == (1, 0, [1, 1, 0, 0])      # the same plane facing away: near, not on
    assert mark_one(GOOD, [ACROSS]) == (1, 0, [1, 1, 0, 0])                  # near but disagreeing: an object
    assert mark_one(GOOD, [ACROSS, ACROSS2]) == (2, -1, [1, 0, 1, 1])        # near two planes: a crease, structure
    assert mark_one(GOOD, [FAR, ACROSS, ACROSS2]) == (3, -1, [1, 0, 1, 1])   # the lowest near j
    assert mark_one(GOOD, [FAR, ON, ON]) == (3, -1, [1, 0, 1, 0])            # the lowest on j
    assert mark_one(GOOD, [ACROSS, FAR, ON]) == (4, -1, [1, 0, 1, 0])        # on beats near, whatever the order
    assert mark_one(GOOD, [FAR] * 15 + [ON]) == (17, -1, [1, 0, 1, 0])       # sixteen planes
    # the band's edge: |r| == band is near
    assert mark_one(GOOD, [[0, 0, 1.0, 0.25], ACROSS]) == (2, -1, [1, 0, 1, 1])
    assert mark_one(GOOD, [[0, 0, 1.0, 0.25], ACROSS], band=0.2499) == (1, 0, [1, 1, 0, 0])
    # the cone: 10 degrees; a plane 9 degrees off agrees, 11 degrees off does not
    for deg, kind in ((9.0, 2), (11.0, 1)):
        n = AR.rotation([0.0, 0.0, math.radians(deg)]) @ DIAG
        assert mark_one(GOOD, [[*n, float(n @ [0.5, 0.5, 0.5])]])[0] == kind, deg
    for bad in (math.nan, 1.0, -1.0):                                        # NaN and saturated corners: no sample
        v = GOOD.astype(np.float64).copy()
        v[1, 0, 1] = bad
        assert mark_one(v, [ON]) == (0, -1, [0, 0, 0, 0]), bad
    for bad in (0.0, math.nan):                                              # an unseen corner
        w = np.ones((2, 2, 2))
        w[0, 1, 0] = bad
        assert mark_one(GOOD, [ON], weights=w) == (0, -1, [0, 0, 0, 0])
    assert mark_one(GOOD, [], weights=2 * np.ones(8), min_weight=2.5) == (0, -1, [0, 0, 0, 0])
    assert mark_one(np.full(8, 0.25), []) == (0, -1, [0, 0, 0, 0])           # no sign change
    assert mark_one(0.5 * (-1.0) ** (I + J + K), []) == (0, -1, [0, 0, 0, 0])   # no gradient
    assert mark_one(GOOD, [[math.nan, 0, 0, 0.0], [0, 0, 1.0, math.nan]]) == (1, 0, [1, 1, 0, 0])   # a NaN is not near


def test_the_restated_labels_are_scipys_components_and_the_table_a_direct_sum():
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(3)
    for shape, p in (((7, 6, 9), 0.15), ((5, 5, 5), 0.5), ((1, 1, 1), 1.0), ((3, 4, 40), 0.08)):
        member = rng.random(shape) < p
        start = np.where(member, np.arange(member.size).reshape(shape), -1).astype(np.int32)
        label = OR.labels(start)
        ref, n = ndimage.label(member, structure=np.ones((3, 3, 3)))
        assert (label >= 0).tolist() == member.tolist()
        pairs = set(zip(label[member].tolist(), ref[member].tolist()))
        assert len(pairs) == n == len({a for a, _ in pairs}) == len({b for _, b in pairs})     # the same partition
        for root in np.unique(label[member]):
            assert root == np.flatnonzero(label.reshape(-1) == root)[0]                       # named by its smallest index
        kind = np.where(member, 1, rng.choice([0, 0, 2, 3, 5, 17], shape)).astype(np.uint8)
        t = OR.table(kind, label)
        roots = np.unique(label[member])
        assert t["root"].tolist() == roots.tolist() and t["sum2"].dtype == np.int64
        for i, root in enumerate(roots):
            c = np.argwhere(label == root)
            assert t["size"][i] == len(c) and t["sum"][i].tolist() == c.sum(0).tolist()
            assert t["sum2"][i].tolist() == [int((c[:, a] * c[:, b]).sum()) for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
            assert t["bbox"][i].tolist() == [*c.min(0), *c.max(0)]
            bits = 0
            for cell in c:
                lo, hi = np.maximum(cell - 1, 0), np.minimum(cell + 2, shape)
                for k in np.unique(kind[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]):
                    if k >= 2:
                        bits |= 1 << (int(k) - 2)
            assert t["touch"][i] == bits
        few = OR.table(kind, label, rows=min(2, len(roots)))
        assert few["root"].tolist() == roots[:2].tolist() and few["size"].tolist() == t["size"][:2].tolist()


def test_the_encoding_orders_as_the_floats_do():
    x = np.array([-math.inf, -3.5, -1e-40, -0.0, 0.0, 1e-40, 2.0, math.inf], F)
    e = OR.encode(x)
    assert (np.diff(e.astype(np.int64)) > 0).all()
    assert e[0] == TO.EXT_EMPTY[1] and e[-1] == TO.EXT_EMPTY[0]
    assert TO.decode_extents(e).tolist() == x.astype(np.float64).tolist()
    assert math.copysign(1.0, TO.decode_extents(e)[3]) == -1.0


# ---- the host steps -----------------------------------------------------------------------------------------------------
def moments(cells):
    c = np.asarray(cells, np.int64)
    pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    return len(c), c.sum(0), np.array([(c[:, a] * c[:, b]).sum() for a, b in pairs])


def cuboid(n0, n1, n2, at=(900, 850, 700)):
    g = np.stack(np.meshgrid(np.arange(n0), np.arange(n1), np.arange(n2), indexing="ij"), -1).reshape(-1, 3)
    return g + np.asarray(at)                                   # far from the origin: the integers are large, and exact


@pytest.mark.parametrize("up_axis", [0, 1, 2])
@pytest.mark.parametrize("up_sign", [1, -1])
def test_axes_from_hand_made_moments(up_axis, up_sign):
    up = np.zeros(3)
    up[up_axis] = up_sign
    a, b = [ax for ax in range(3) if ax != up_axis]
    for long_ax, short_ax in ((a, b), (b, a)):
        n = [0, 0, 0]
        n[up_axis], n[long_ax], n[short_ax] = 9, 12, 4
        axes, elongation = TO.object_axes(*moments(cuboid(*n)), up)
        want = np.zeros(3)
        want[long_ax] = 1.0
        assert axes[0].tolist() == up.tolist() and np.abs(axes[1] - want).max() < 1e-12
        assert np.abs(axes[2] - np.cross(up, want)).max() < 1e-12
        assert elongation == pytest.approx((12 ** 2 - 1) / (4 ** 2 - 1), rel=1e-12)      # variances of n cells: (n^2 - 1) / 12
    C = TO.covariance_integers(*moments(cuboid(2, 3, 5)))
    assert all(isinstance(v, int) for row in C for v in row)
    assert [C[i][i] for i in range(3)] == [30 * 30 * (k * k - 1) // 12 for k in (2, 3, 5)] and C[0][1] == C[1][2] == 0
    # a square footprint: no long axis to speak of, but a frame all the same; one cell and a column: elongation inf
    axes, elongation = TO.object_axes(*moments(cuboid(5, 5, 5)), up)
    assert elongation == pytest.approx(1.0, rel=1e-9) and np.abs(axes @ axes.T - np.eye(3)).max() < 1e-12
    assert np.linalg.det(axes) == pytest.approx(1.0) and axes[1][int(np.argmax(np.abs(axes[1])))] > 0
    n = [1, 1, 1]
    n[up_axis] = 6
    for cells in (cuboid(1, 1, 1), cuboid(*n)):
        axes, elongation = TO.object_axes(*moments(cells), up)
        assert elongation == math.inf and np.abs(axes @ axes.T - np.eye(3)).max() < 1e-12


def test_the_sign_rule_and_a_tilted_up():
    line = np.array([[k, 20 - k, 5] for k in range(12)])        # along (1, -1, 0): a tie of magnitudes, the lowest axis wins
    axes, elongation = TO.object_axes(*moments(line), np.array([0.0, 0.0, 1.0]))
    assert np.abs(axes[1] - np.array([1.0, -1.0, 0.0]) / math.sqrt(2)).max() < 1e-12 and elongation == math.inf
    axes, _ = TO.object_axes(*moments(np.array([[k, 3 * k, 0] for k in range(9)])), np.array([0.0, 0.0, -1.0]))
    assert np.abs(axes[1] - np.array([1.0, 3.0, 0.0]) / math.sqrt(10)).max() < 1e-12       # the largest component: positive
    axes, _ = TO.object_axes(*moments(np.array([[-k, 3 * k + 40, 0] for k in range(9)])), np.array([0.0, 0.0, 1.0]))
    assert np.abs(axes[1] - np.array([-1.0, 3.0, 0.0]) / math.sqrt(10)).max() < 1e-12
    up = AR.rotation([0.3, -0.2, 0.1]) @ np.array([0.0, 0.0, 1.0])
    axes, _ = TO.object_axes(*moments(cuboid(10, 3, 4)), up)
    assert np.abs(axes @ axes.T - np.eye(3)).max() < 1e-12 and abs(axes[1] @ up) < 1e-12 and axes[1][0] > 0.9
    E = TO.level_basis(up)
    assert np.abs(E @ up).max() < 1e-15 and np.abs(E @ E.T - np.eye(2)).max() < 1e-15


def test_structure_planes_is_the_floor_and_the_large_planes():
    P = PC.plane
    small, wall, floor, face = P([0, 0, -1], -2.0, 50), P([0, 0, -1], -4.0, 500), P([0, -1, 0], -1.2, 400), P([1, 0, 0], 0.5, 60)
    for p, area in ((small, 0.8), (wall, 8.4), (floor, 24.7), (face, 1.99)):
        p["area_m2"] = area
    planes = [wall, floor, small, face]
    assert TO.structure_planes(planes, floor)[1] == [1, 0] and TO.structure_planes(planes)[1] == [0, 1]
    assert TO.structure_planes(planes, small)[1] == [2, 0, 1]                  # a floor is structure whatever its area
    assert TO.structure_planes(planes, floor, min_area_m2=1.99)[1] == [1, 0, 3]
    assert TO.structure_planes(planes, floor, min_area_m2=0.0)[0] == [floor, wall, small, face]
    assert TO.structure_planes([], None) == ([], [])
    many = [dict(wall) for _ in range(20)]
    assert len(TO.structure_planes(many)[0]) == 16
    for bad in (dict(floor=dict(floor)), dict(min_area_m2=-1.0), dict(min_area_m2=math.nan)):
        with pytest.raises(ValueError, match="structure_planes"):
            TO.structure_planes(planes, **bad)


def same_boxes(a, b):
    assert len(a) == len(b)
    for p, q in zip(a, b):
        assert set(p) == set(q)
        for key in ("root", "cells", "touches", "bbox_cells", "elongation"):
            assert p[key] == q[key], key
        assert (p["above_m"] is None) == (q["above_m"] is None)
        for key in ("axes", "centre", "size_m") + (("above_m",) if p["above_m"] is not None else ()):
            x, y = (np.ascontiguousarray(v[key], np.float64).view(np.int64) for v in (p, q))
            assert np.array_equal(x, y), key


def test_moved_objects_and_the_text_round_trip():
    w = world("tilted")
    boxes = w["objects"].boxes
    T = TP.upright_transform(w["floor"], 2, 1)
    moved = TO.moved_objects(w["objects"], T)
    for b, m in zip(boxes, moved):
        assert np.abs(m["axes"][0] - [0, 0, 1]).max() < 1e-12                # up is the map's z
        assert np.abs(m["centre"] - (T[:3, :3] @ b["centre"] + T[:3, 3])).max() < 1e-15
        assert m["centre"][2] == pytest.approx(0.5 * (b["above_m"][0] + b["above_m"][1]), abs=1e-9)
        assert m["size_m"] is b["size_m"] and m["cells"] == b["cells"] and m["touches"] == b["touches"]
    back = TO.moved_objects(moved, np.linalg.inv(T))
    for b, m in zip(boxes, back):
        assert np.abs(m["axes"] - b["axes"]).max() < 1e-12 and np.abs(m["centre"] - b["centre"]).max() < 1e-12
    with pytest.raises(ValueError, match="moved_objects"):
        TO.moved_objects(boxes, 2 * np.eye(4))
    bare = OR.find_objects(w["vol"], w["structure"], up=w["up"]).boxes        # a bare vector: no above_m
    assert all(b["above_m"] is None for b in bare) and len(bare) == 3
    for args in ((boxes, None), (boxes, moved), (bare, None), ([], None), ([], [])):
        text = TO.objects_text(*args)
        got, got_moved = TO.parse_objects(text)
        assert TO.objects_text(got, got_moved) == text
        same_boxes(got, args[0])
        assert (got_moved is None) == (args[1] is None)
        if args[1] is not None:
            same_boxes(got_moved, args[1])
    text = TO.objects_text(boxes, moved)
    for bad in ("", "something else\n", text + "1 2 3\n", text + "frame\tmap\nobjects\t0\n", text.replace("objects\t3", "objects\t4", 1)):
        with pytest.raises(ValueError, match="objects.txt"):
            TO.parse_objects(bad)


def test_bad_arguments_are_refused_before_the_library(monkeypatch):
    from go_slam_amd import _lib
    from go_slam_amd.tsdf import TSDFVolume

    def unloaded():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "lib", unloaded)
    vol = TSDFVolume.__new__(TSDFVolume)
    vol.voxel, vol.lo, vol.dims, vol.trunc, vol.max_weight, vol.device = VOXEL, np.array(LO), DIMS, TRUNC, 64.0, "cuda:0"
    vol.tsdf = vol.weight = vol.colors = None
    floor = PC.plane([0, -1, 0], -1.2, 100)
    for bad in (dict(planes=[]), dict(planes=None), dict(planes=[floor] * 17), dict(planes=[{"normal": [0, 0, 2.0], "offset": 0.0}]),
                dict(up=[0, 0, 0]), dict(up=[1, 2]), dict(up={"normal": [0, 0, 1.0]}), dict(up={"normal": [0, 3.0, 0], "offset": 1.0}),
                dict(cone_deg=0), dict(cone_deg=90), dict(cone_deg=math.nan), dict(band=0.0), dict(band=-1.0),
                dict(band=math.inf), dict(min_cells=0), dict(min_cells=2.5), dict(min_weight=math.nan),
                dict(min_weight=math.inf), dict(max_sweeps=0), dict(max_sweeps=1.5), dict(max_sweeps=True)):
        with pytest.raises(ValueError, match="TSDFVolume.find_objects"):
            vol.find_objects(**dict(dict(planes=[floor]), **bad))
    with pytest.raises(ValueError, match="no TSDFVolume"):
        TO.find_objects(types.SimpleNamespace(tsdf=None), [floor])
    args = TO.find_arguments("t", VOXEL, [], up=[0, 0, 2.0])                 # no planes, but an up: fine
    assert args["planes"].shape == (0, 4) and args["up"].tolist() == [0, 0, 1] and args["up_offset"] is None
    args = TO.find_arguments("t", VOXEL, [floor])
    assert args["up"].tolist() == [0, -1, 0] and args["up_offset"] == -1.2 and args["band"] == VOXEL and args["cos2"] == COS2


# ---- the room ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, areas", [("straight", (24.7, 8.44, 0.81, 0.80)), ("tilted", (17.5, 7.09, 0.84, 0.81))])
def test_structure_planes_keeps_the_floor_and_the_wall_of_the_room(name, areas):
    w = world(name)
    planes = w["planes"]
    print(name, "areas:", [round(p["area_m2"], 3) for p in planes], "structure:", w["index"])
    assert len(planes) == 4 and w["floor"] is not None
    assert [p["area_m2"] for p in planes] == pytest.approx(areas, rel=0.02)
    truth = PC.truth(w["M"])
    assert len(w["structure"]) == 2 and w["structure"][0] is w["floor"]
    assert float(w["structure"][0]["normal"] @ truth["floor"][0]) > 0.999 and float(w["structure"][1]["normal"] @ truth["wall"][0]) > 0.999
    left = [p for i, p in enumerate(planes) if i not in w["index"]]
    assert len(left) == 2 and all(p["area_m2"] < 1.0 for p in left)           # the two large faces of box B
    face = w["M"][:3, :3] @ TURN_B @ np.array([0.0, 0.0, 1.0])
    assert all(abs(float(p["normal"] @ face)) > 0.99 for p in left)


@pytest.mark.parametrize("name, counts", [("straight", (2882, 2193, 72)), ("tilted", (2955, 2207, 49))])
def test_the_restated_pipeline_finds_the_three_things(name, counts):
    """Exactly three objects of at least 16 cells, inside the bounds the geometry gives (`check_boxes`).  counts: samples,
    structure cells, crease cells (structure that is on no plane; in the tilted world 69 cells are near both planes and 20 of
    them are on one)."""
    w = world(name)
    obj = w["objects"]
    print(name, "counts:", obj.counts.tolist(), "clusters:", obj.n_clusters, "sizes:", sorted(obj.size.tolist(), reverse=True)[:8])
    assert obj.counts[0] == obj.counts[1] + obj.counts[2] and obj.counts[3] <= obj.counts[2]
    assert (obj.counts[0], obj.counts[2], obj.counts[3]) == counts
    assert obj.counts[1] == obj.size.sum() and obj.n_clusters == len(obj.root) >= 3
    assert [b["cells"] for b in obj.boxes] == sorted((b["cells"] for b in obj.boxes), reverse=True)
    check_boxes(obj.boxes, w)
    again = OR.find_objects(w["vol"], w["structure"])
    assert TO.objects_text(again.boxes) == TO.objects_text(obj.boxes)


def test_without_the_crease_rule_or_the_area_policy_the_room_goes_wrong():
    """One plane alone leaves the crease along the floor's edge at the wall as a long thin object that touches the floor;
    with box B's faces as structure the box falls apart."""
    w = world("straight")
    vol = w["vol"]
    s = PR.samples(vol)
    planes4 = np.array([[*p["normal"], p["offset"]] for p in w["structure"]])
    both = OR.mark(vol, planes4, COS2, VOXEL, s=s)
    crease = (both["kind"] >= 2) & (OR.mark(vol, planes4[:1], COS2, VOXEL, s=s)["kind"] == 1) & \
        (OR.mark(vol, planes4[1:], COS2, VOXEL, s=s)["kind"] == 1)
    print("crease cells:", int(crease.sum()), "counted:", int(both["counts"][3]))
    assert crease.sum() == both["counts"][3] == 72
    cells = np.argwhere(crease)
    assert np.ptp(cells[:, 0]) * VOXEL > 4.0 and np.ptp(cells[:, 1]) <= 2 and np.ptp(cells[:, 2]) <= 2     # 4.5 m along x
    label = OR.labels(np.where(crease, np.arange(crease.size).reshape(crease.shape), -1).astype(np.int32))
    assert len(np.unique(label[crease])) == 1                   # one thin piece
    everything, _ = TO.structure_planes(w["planes"], w["floor"], min_area_m2=0.0)
    apart = OR.find_objects(vol, everything)
    near_b = [b for b in apart.boxes if np.linalg.norm(b["centre"] - THINGS["box_b"][0]) < 0.8]
    print("with every plane as structure:", [(b["cells"], np.round(b["centre"], 2).tolist()) for b in apart.boxes])
    assert len(apart.boxes) != 3 or len(near_b) != 1 or near_b[0]["cells"] < 0.7 * match(w["objects"].boxes, w["M"])["box_b"]["cells"]
