"""The distance-field contract (include/goslam_hip.h, gs_esdf_*) on the CPU: tests/esdf_restatement.py against an
independent implementation (scipy.ndimage.distance_transform_edt), the kernels' early-exit loop against the plain
windowed minimum, a closed form, the field's Lipschitz property, and the Python surface that needs no launch."""
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import esdf_restatement as ER                                  # noqa: E402

VOXEL = 0.125


def sphere_field(dims=(19, 23, 17), centre=(8.3, 11.1, 7.6), radius=5.4):
    g = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in dims], indexing="ij")
    r = np.sqrt(sum((g[a] - centre[a]) ** 2 for a in range(3)))
    return np.clip((r - radius) / 4.0, -1, 1).astype(np.float32), np.ones(dims, np.float32)      # solid inside


def oblique_field(dims=(21, 9, 30)):
    g = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in dims], indexing="ij")
    s = (0.48 * g[0] + 0.6 * g[1] + 0.64 * g[2]) - 14.3
    return np.clip(-s / 4.0, -1, 1).astype(np.float32), np.ones(dims, np.float32)


def random_field(dims=(13, 11, 17), seed=11):
    g = np.random.default_rng(seed)
    tsdf = g.uniform(-1, 1, dims).astype(np.float32)
    weight = (g.random(dims) >= 0.3).astype(np.float32) * 2.0                                      # 30 % unknown
    return tsdf, weight


def empty_field(dims=(7, 5, 9)):
    return np.ones(dims, np.float32), np.ones(dims, np.float32)


def tiny_field():
    tsdf = np.ones((2, 2, 2), np.float32)
    tsdf[1, 0, 1] = -0.5
    return tsdf, np.ones((2, 2, 2), np.float32)


CASES = {"sphere": sphere_field, "oblique": oblique_field, "random": random_field, "empty": empty_field,
         "tiny": tiny_field}


def edt_d2(site, R):
    """The squared distance to the nearest site by scipy's exact Euclidean transform, under the FAR rule.  rint(sqrt(v)^2)
    == v for every integer up to 3 * 1023^2 in float64.  Without any site the transform has nothing to measure to:
    every point is FAR."""
    from scipy.ndimage import distance_transform_edt
    if not site.any():
        return np.full(site.shape, ER.FAR, np.int32)
    d2 = np.rint(distance_transform_edt(~site) ** 2).astype(np.int64)
    return np.where(d2 > R * R, ER.FAR, d2).astype(np.int32)


def test_rint_of_a_squared_root_gives_the_integer_back():
    v = np.arange(3 * 1023 ** 2 + 1, dtype=np.float64)
    assert np.array_equal(np.rint(np.sqrt(v) ** 2), v)


@pytest.mark.parametrize("R", [3, 1023])
@pytest.mark.parametrize("name", list(CASES))
def test_restated_d2_is_the_exact_euclidean_transform(name, R):
    tsdf, weight = CASES[name]()
    ref = ER.build(tsdf, weight, R, VOXEL)
    assert ref["site"].any() == (name != "empty")
    if name == "random":
        assert (ref["state"] == 0).mean() > 0.2 and ref["site"].mean() > 0.3
    assert np.array_equal(ref["d2"], edt_d2(ref["site"], R))
    assert (ref["d2"][ref["site"]] == 0).all()
    if R == 3 and name in ("sphere", "oblique"):
        assert (ref["d2"] == ER.FAR).any() and (ref["d2"] == 9).any()
    if R == 1023 and name != "empty":
        assert (ref["d2"] != ER.FAR).all()


@pytest.mark.parametrize("R", [1, 3, 1023])
@pytest.mark.parametrize("name", list(CASES))
def test_the_early_exit_loop_is_the_plain_windowed_minimum(name, R):
    tsdf, weight = CASES[name]()
    site = ER.site_mask(ER.states(tsdf, weight))
    f = np.where(site, 0, ER.INF).astype(np.int64)
    for axis in (2, 1, 0):                                     # pass by pass, on the inputs the passes really see
        plain, early = ER.window_min(f, axis, R), ER.early_exit_min(f, axis, R)
        assert np.array_equal(plain, early)
        f = plain
    assert np.array_equal(ER.squared_distance(site, R, ER.early_exit_min), ER.squared_distance(site, R))


def test_states_and_sites_follow_the_order_of_the_contract():
    tsdf = np.array([[[0.5, -0.5, np.nan, -0.5, -0.5, 0.5]]], np.float32).repeat(2, 0).repeat(2, 1)
    weight = np.array([[[1.0, 1.0, 1.0, np.nan, 0.5, 1.0]]], np.float32).repeat(2, 0).repeat(2, 1)
    state = ER.states(tsdf, weight, 1.0)
    assert state[0, 0].tolist() == [1, 2, 1, 0, 0, 1]          # NaN tsdf is free, NaN or small weight unknown
    site = ER.site_mask(state)
    assert site[0, 0].tolist() == [True, True, True, False, False, False]      # unknown points separate, never sites


@pytest.mark.parametrize("R", [3, 1023])
def test_axis_aligned_plane_has_the_closed_form(R):
    """Solid from layer 6 of z on: the sites are layers 5 and 6, and dist is exactly voxel * layers to the nearer one,
    negative behind the plane, capped at R."""
    dims = (5, 4, 16)
    tsdf = np.ones(dims, np.float32)
    tsdf[:, :, 6:] = -1.0
    ref = ER.build(tsdf, np.ones(dims, np.float32), R, VOXEL)
    k = np.arange(16)
    layers = np.where(k <= 5, 5 - k, k - 6)
    want = np.where(k <= 5, 1.0, -1.0) * VOXEL * np.minimum(layers, R)
    assert np.array_equal(ref["dist"], np.broadcast_to(want.astype(np.float32), dims))
    assert np.array_equal(ref["d2"][0, 0], np.where(layers > R, ER.FAR, layers ** 2))


@pytest.mark.parametrize("R", [3, 1023])
@pytest.mark.parametrize("name", ["sphere", "oblique", "random"])
def test_dist_changes_by_at_most_a_voxel_between_neighbours_of_one_sign(name, R):
    """The distance to a set is 1-Lipschitz and the cap keeps that; dist is that distance rounded twice (sqrtf, the
    multiply), so two neighbours of the same sign differ by a voxel plus at most 2 ulps of the larger magnitude each."""
    tsdf, weight = CASES[name]()
    ref = ER.build(tsdf, weight, R, VOXEL)
    d = ref["dist"].astype(np.float64)
    neg = ref["state"] == 2
    checked = 0
    for axis in range(3):
        a = [slice(None)] * 3
        b = [slice(None)] * 3
        a[axis], b[axis] = slice(0, -1), slice(1, None)
        a, b = tuple(a), tuple(b)
        same = neg[a] == neg[b]
        slack = 4 * 2.0 ** -24 * np.maximum(np.abs(d[a]), np.abs(d[b]))
        assert (np.abs(d[a] - d[b])[same] <= (VOXEL + slack)[same]).all()
        checked += int(same.sum())
    assert checked > 1000
    assert (ref["dist"][neg] <= 0).all() and (ref["dist"][~neg] >= 0).all()
    assert np.abs(ref["dist"]).max() <= np.float32(VOXEL) * np.float32(R)


def test_query_restatement_on_a_linear_field():
    """dist = voxel * (k - 2) along z is reproduced exactly by the trilinear interpolant at dyadic points, with gradient
    (0, 0, 1); points on the last lattice plane, outside, NaN and inf are invalid and read zero."""
    dims = (4, 5, 9)
    dist = np.broadcast_to((VOXEL * (np.arange(9) - 2.0)).astype(np.float32), dims).copy()
    state = np.ones(dims, np.uint8)
    state[3, 4, 8] = 0
    lo = (-1.0, 0.5, 2.0)
    pts = np.array([[-1.0 + 1.25 * VOXEL, 0.5 + 2.5 * VOXEL, 2.0 + 3.75 * VOXEL],
                    [-1.0 + 2.5 * VOXEL, 0.5 + 3.5 * VOXEL, 2.0 + 7.5 * VOXEL],        # the cell with the unknown corner
                    [-1.0 + 3 * VOXEL, 0.6, 2.1], [-1.0, 0.5, 2.0 + 8 * VOXEL],          # on the last x / z plane
                    [-1.01, 0.6, 2.1], [np.nan, 0.6, 2.1], [0.0, np.inf, 2.1], [0.0, 0.6, -np.inf]], np.float32)
    d, g, valid, known = ER.query(dist, state, lo, VOXEL, pts)
    assert valid.tolist() == [True, True] + [False] * 6 and known.tolist() == [True] + [False] * 7
    assert d[0] == np.float32(VOXEL * 1.75) and d[1] == np.float32(VOXEL * 5.5)
    assert np.array_equal(g[:2], np.array([[0, 0, 1], [0, 0, 1]], np.float32))
    assert not d[2:].any() and not g[2:].any()


def test_slice_restatement_on_a_hand_made_slab():
    state = np.ones((2, 3, 4), np.uint8)
    d2 = np.full((2, 3, 4), 9, np.int32)
    dist = np.full((2, 3, 4), 3 * VOXEL, np.float32)
    state[0, 0, 1] = 2
    dist[0, 0, 1] = -0.0
    d2[0, 1, 2] = 4
    dist[0, 1, 2] = 2 * VOXEL
    state[1, 2, :3] = 0
    cells, clearance = ER.occupancy_slice(state, d2, dist, 2, 0, 3, 4, 2)
    assert cells.tolist() == [[0, 0, 254], [254, 254, 205]]
    assert clearance[0, 1] == np.float32(2 * VOXEL) and clearance[1, 0] == np.float32(3 * VOXEL)
    cells, _ = ER.occupancy_slice(state, d2, dist, 2, 3, 3, 0, 1)          # the top layer alone: nothing solid, all seen
    assert (cells == 254).all()
    cells, _ = ER.occupancy_slice(state, d2, dist, 0, 0, 0, 0, 1)          # x up: image [ny, nz]
    assert cells.shape == (3, 4) and cells[0, 1] == 0 and cells[1, 2] == 254


# ---- the Python surface ---------------------------------------------------------------------------------------------
def cpu_volume():
    from go_slam_amd.tsdf import TSDFVolume
    return TSDFVolume([[-1.0, 1.0], [-0.5, 0.5], [0.0, 2.0]], VOXEL, device="cpu")          # 17 x 9 x 17


def cpu_field(radius=8):
    from go_slam_amd.tsdf import ESDF
    dims = (17, 9, 17)
    return ESDF(torch.ones(dims, dtype=torch.uint8), torch.zeros(dims, dtype=torch.int32), torch.zeros(dims), [-1.0, -0.5, 0.0],
                VOXEL, dims, radius)


def test_bad_arguments_raise_before_any_library_call(monkeypatch):
    from go_slam_amd import _lib

    def no_library():
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(_lib, "lib", no_library)
    vol = cpu_volume()
    for bad in (0.0, -1.0, math.nan, math.inf, 1023 * VOXEL + 1e-6, 1e9):
        with pytest.raises(ValueError, match="max_distance"):
            vol.esdf(bad)
    with pytest.raises(ValueError, match="min_weight"):
        vol.esdf(1.0, min_weight=math.nan)
    field = cpu_field()
    for height in ((0.26, 0.37), (2.01, 3.0), (-2.0, -0.01), (1.0, 0.5), (math.nan, 1.0)):
        with pytest.raises(ValueError, match="height|layer"):
            field.occupancy_slice(2, height)
    with pytest.raises(ValueError, match="robot_radius"):
        field.occupancy_slice(2, (0.0, 1.0), robot_radius=8 * VOXEL + 1e-6)
    with pytest.raises(ValueError, match="robot_radius"):
        field.occupancy_slice(2, (0.0, 1.0), robot_radius=-0.1)
    for axis in (-1, 3, 1.0, None):
        with pytest.raises(ValueError, match="up_axis"):
            field.occupancy_slice(axis, (0.0, 1.0))
    with pytest.raises(ValueError, match="known_fraction"):
        field.occupancy_slice(2, (0.0, 1.0), known_fraction=1.5)
    for points in (torch.zeros(3), torch.zeros(4, 2), torch.zeros(2, 3, 1)):
        with pytest.raises(ValueError, match=r"\[N,3\]"):
            field.query(points)


def test_slice_arguments_follow_the_documented_rounding():
    field = cpu_field()
    # z layers at 0, 0.125, ..., 2: [0.26, 1.0] holds layers 3 .. 8
    assert field.slice_arguments(2, (0.26, 1.0), 0.0, 0.5) == (2, 3, 8, 0, 3)
    assert field.slice_arguments(2, (-5.0, 5.0), 2.5 * VOXEL, 1.0) == (2, 0, 16, 6, 17)
    assert field.slice_arguments(1, (-math.inf, math.inf), 8 * VOXEL, 0.0) == (1, 0, 8, 64, 0)
    assert field.slice_arguments(0, (0.0, 0.0), 0.0, 0.01) == (0, 8, 8, 0, 1)


def test_map_files_round_trip_bit_for_bit(tmp_path):
    from go_slam_amd import tsdf
    g = np.random.default_rng(5)
    cells = g.choice(np.array([0, 205, 254], np.uint8), size=(7, 4))
    grid = {"cells": torch.from_numpy(cells), "origin": (-1.0 - 0.1 / 3, 0.7 / 3), "resolution": 0.1 / 3, "axes": (0, 2)}
    tsdf.save_map(str(tmp_path / "map"), grid)
    raw = open(tmp_path / "map" / "occupancy.pgm", "rb").read()
    assert raw.startswith(b"P5\n7 4\n255\n") and len(raw) == 11 + 28
    rows = np.frombuffer(raw[11:], np.uint8).reshape(4, 7)
    for r in range(4):
        assert np.array_equal(rows[r], cells[:, 3 - r])       # file row r is v = n_v - 1 - r, the column is u
    text = open(tmp_path / "map" / "occupancy.yaml").read().splitlines()
    assert [l.split(":")[0] for l in text] == ["image", "resolution", "origin", "negate", "occupied_thresh", "free_thresh"]
    assert text[0] == "image: occupancy.pgm" and text[3:] == ["negate: 0", "occupied_thresh: 0.65", "free_thresh: 0.196"]
    back = tsdf.load_map(str(tmp_path / "map"))
    assert np.array_equal(back["cells"], cells) and back["cells"].dtype == np.uint8
    assert back["origin"] == grid["origin"] and back["resolution"] == grid["resolution"]


def test_clearance_text_round_trips_bit_for_bit():
    from go_slam_amd import tsdf
    res = {"clearance_min_m": -0.1 / 3, "clearance_mean_m": 2.0 / 7, "n_inside": 2, "n_unknown": 1, "n_poses": 16}
    text = tsdf.clearance_text(res)
    assert text.splitlines()[2] == f"clearance_min_m\t{-0.1 / 3!r}"
    assert tsdf.parse_clearance(text) == res
    nan = dict(res, clearance_min_m=math.nan, clearance_mean_m=math.nan, n_unknown=16)
    back = tsdf.parse_clearance(tsdf.clearance_text(nan))
    assert math.isnan(back["clearance_min_m"]) and math.isnan(back["clearance_mean_m"]) and back["n_unknown"] == 16
    with pytest.raises(ValueError):
        tsdf.parse_clearance("something else\n")
