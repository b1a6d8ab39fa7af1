"""View gain without a GPU (go_slam_amd/view.py, tests/view_gain_restatement.py): the restatement's walk against an
independent definition in exact rationals -- the cells whose cubes the ray crosses -- with many exact corner ties, the
range as a prefix and the tight box against the full one; the hand cases that tests/test_view_gain_gpu.py runs on the
kernel too; the camera's rays; the choice rule with every tie; the text round trip; and every ValueError before the
library is reached."""
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

import view_gain_restatement as VR                             # noqa: E402
from go_slam_amd import tsdf, view                             # noqa: E402

DIMS = (9, 11, 13)


def random_rays(n_small=160, n_full=120, seed=0):
    """Directions with components from [-6, 6] (many exact ties) and from the whole range, the axes and diagonals."""
    rng = np.random.default_rng(seed)
    small = rng.integers(-6, 7, size=(n_small, 3))
    full = rng.integers(-VR.MAX_DIR, VR.MAX_DIR + 1, size=(n_full, 3))
    special = [(1, 0, 0), (0, -1, 0), (0, 0, 1), (1, 1, 0), (-1, 0, 1), (0, 1, -1), (1, 1, 1), (-1, -1, -1), (1, -1, 1),
               (VR.MAX_DIR, VR.MAX_DIR, VR.MAX_DIR), (VR.MAX_DIR, -VR.MAX_DIR, 1), (2, 4, 6), (3, -3, 0)]
    d = np.concatenate([small, full, np.array(special)])
    return d[(d != 0).any(axis=1)]


def crossing(origin, d, dims):
    """{cell: (t_in, t_out)} in exact rationals for every cell of the lattice whose closed cube c + [-1/2, 1/2]^3 meets the
    ray origin + t d, t >= 0: the independent definition."""
    spans = []
    for a in range(3):
        per = {}
        for c in range(dims[a]):
            if d[a] == 0:
                if c == origin[a]:
                    per[c] = (Fraction(0), None)                  # the whole ray
            else:
                t = sorted((Fraction(2 * (c - origin[a]) - 1, 2 * d[a]), Fraction(2 * (c - origin[a]) + 1, 2 * d[a])))
                if t[1] >= 0:
                    per[c] = (max(t[0], Fraction(0)), t[1])
        spans.append(per)
    out = {}
    for c0, (lo0, hi0) in spans[0].items():
        for c1, (lo1, hi1) in spans[1].items():
            for c2, (lo2, hi2) in spans[2].items():
                lo = max(lo0, lo1, lo2)
                his = [h for h in (hi0, hi1, hi2) if h is not None]
                hi = min(his)                                     # d != 0: at least one axis bounds it
                if lo <= hi:
                    out[(c0, c1, c2)] = (lo, hi)
    return out


def test_walk_equals_the_cells_the_ray_crosses_in_exact_rationals():
    rng = np.random.default_rng(1)
    ties = 0
    for d in random_rays():
        d = tuple(int(v) for v in d)
        o = tuple(int(rng.integers(0, n)) for n in DIMS)
        cells = VR.walk(o, d, DIMS)
        assert cells[0] == o and len(set(cells)) == len(cells)
        for p, q in zip(cells, cells[1:]):                        # one step on one axis, along the ray
            step = [q[a] - p[a] for a in range(3)]
            assert sorted(abs(s) for s in step) == [0, 0, 1]
            a = [abs(s) for s in step].index(1)
            assert step[a] * d[a] > 0
        meets = crossing(o, d, DIMS)
        through = {c for c, (lo, hi) in meets.items() if lo < hi}
        assert through <= set(cells), (o, d)                      # crossed over a positive length: visited
        assert set(cells) <= set(meets), (o, d)                   # visited: the closed cube meets the ray
        ties += len(set(cells) - through)
        order = [meets[c][0] for c in cells]
        assert order == sorted(order)                             # and in the order the ray enters them
    assert ties > 100                                             # the corner ties were there


def test_a_finite_range_yields_a_prefix_and_the_tight_box_clips_nothing():
    rng = np.random.default_rng(2)
    dims = (41, 41, 41)
    rays = random_rays(seed=3)
    for d in rays:
        d = tuple(int(v) for v in d)
        for lattice, o in ((DIMS, tuple(int(rng.integers(0, n)) for n in DIMS)), (dims, (20, 20, 20))):
            whole = VR.walk(o, d, lattice)
            for r in (1, 2, 5, 12, 20):
                near = VR.walk(o, d, lattice, range2=r * r)
                beyond = [i for i, c in enumerate(whole) if sum((c[a] - o[a]) ** 2 for a in range(3)) > r * r]
                assert near == whole[:beyond[0] if beyond else len(whole)]
                assert VR.walk(o, d, lattice, r * r, VR.full_box(r)) == near
                assert VR.walk(o, d, lattice, r * r, view.view_box([d], r)) == near, (o, d, r)
    for r in (1, 7, 20):                                          # one box for a whole set of rays
        box = view.view_box(rays, r)
        assert all(box[a] <= 0 <= box[3 + a] <= r + 2 and box[a] >= -r - 2 for a in range(3))
        for d in rays[::7]:
            assert VR.walk((20, 20, 20), d, dims, r * r, box) == VR.walk((20, 20, 20), d, dims, r * r)
    # the reach is the stated formula, one-sided
    assert view.view_box([(3, 0, 0)], 10) == (0, 0, 0, 12, 0, 0)
    assert view.view_box([(0, -5, 0), (0, 0, 0)], 10) == (0, -12, 0, 0, 0, 0)
    assert view.view_box([(3, 4, 0)], 9) == (0, 0, 0, 7, 9, 0)     # floor(10 * 0.6 + 1), floor(10 * 0.8 + 1)
    assert view.view_box([(0, 0, 0)], 9) == (0, 0, 0, 0, 0, 0)


# ---- hand cases (tests/test_view_gain_gpu.py runs them on the kernel) -------------------------------------------------
def corridor():
    """3 x 3 x 12, solid but for the middle row: free at 0..7, unknown at 8 and 9, solid from 10."""
    state = np.full((3, 3, 12), 2, dtype=np.uint8)
    state[1, 1, :8] = 1
    state[1, 1, 8:10] = 0
    return state


def cases():
    """(name, state, origins, dirs, range_cells, max_unknown, box or None, want [V,4])"""
    free = np.ones((3, 3, 12), dtype=np.uint8)
    along = [(0, 0, 1)]
    plane = np.ones((8, 8, 1), dtype=np.uint8)
    solid_origin = np.ones((3, 3, 3), dtype=np.uint8)
    solid_origin[1, 1, 1] = 7
    return [
        ("an axis ray in a corridor: the solid cell is counted and ends it, unknown cells do not", corridor(), [(1, 1, 0)],
         along, 20, 0, None, [(2, 8, 1, 11)]),
        ("max_unknown 1 ends it on that cell", corridor(), [(1, 1, 0)], along, 20, 1, None, [(1, 8, 0, 9)]),
        ("max_unknown 2 ends it on the second", corridor(), [(1, 1, 0)], along, 20, 2, None, [(2, 8, 0, 10)]),
        ("max_unknown 3 is never reached", corridor(), [(1, 1, 0)], along, 20, 3, None, [(2, 8, 1, 11)]),
        ("offset 5 is in at range 5 and offset 6 is out", free, [(1, 1, 0)], along, 5, 0, None, [(0, 6, 0, 6)]),
        ("(3,4,0) lies at exactly range2 = 25 and is in; (3,5,0) is out", plane, [(0, 0, 0)], [(3, 4, 0)], 5, 0, None,
         [(0, 8, 0, 8)]),
        ("the lattice border ends it", np.ones((1, 1, 5), dtype=np.uint8), [(0, 0, 2)], [(0, 0, 1), (0, 0, -1)], 10, 0, None,
         [(0, 5, 0, 5)]),
        ("a box clips it", free, [(1, 1, 0)], along, 10, 0, (0, 0, 0, 0, 0, 3), [(0, 4, 0, 4)]),
        ("duplicate rays change nothing", corridor(), [(1, 1, 0)], along * 3, 20, 0, None, [(2, 8, 1, 11)]),
        ("an origin outside the lattice gives zeros", corridor(), [(-1, 1, 0), (1, 1, 12), (1, 3, 0), (1, 1, 0)], along, 20,
         0, None, [(0, 0, 0, 0), (0, 0, 0, 0), (0, 0, 0, 0), (2, 8, 1, 11)]),
        ("a solid origin", solid_origin, [(1, 1, 1)], [(1, 0, 0), (0, -1, 1)], 5, 0, None, [(0, 0, 1, 1)]),
        ("an all-zero direction casts nothing", free, [(1, 1, 0)], [(0, 0, 0)], 5, 0, None, [(0, 0, 0, 0)]),
        ("a diagonal's ties go to the lower axis", np.ones((4, 4, 1), dtype=np.uint8), [(0, 0, 0)], [(1, 1, 0)], 10, 0, None,
         [(0, 7, 0, 7)]),
        ("two rays share their first cells", corridor(), [(1, 1, 2)], [(0, 0, 1), (0, 0, -1), (1, 0, 0)], 20, 0, None,
         [(2, 8, 2, 12)]),
    ]


@pytest.mark.parametrize("case", cases(), ids=lambda c: c[0])
def test_hand_cases(case):
    _, state, origins, dirs, r, max_unknown, box, want = case
    got = VR.gains(state, origins, dirs, r * r, max_unknown, box)
    assert got.tolist() == [list(w) for w in want]
    assert (got[:, :3].sum(axis=1) == got[:, 3]).all()
    if box is None:                                               # the tight box and the full box change nothing
        assert np.array_equal(VR.gains(state, origins, dirs, r * r, max_unknown, view.view_box(dirs, r)), got)
        assert np.array_equal(VR.gains(state, origins, dirs, r * r, max_unknown, VR.full_box(r)), got)


def test_the_diagonal_tie_visits_the_lower_axis_first():
    assert VR.walk((0, 0, 0), (1, 1, 0), (4, 4, 1))[:4] == [(0, 0, 0), (1, 0, 0), (1, 1, 0), (2, 1, 0)]
    assert VR.walk((1, 1, 1), (-1, -1, -1), (3, 3, 3)) == [(1, 1, 1), (0, 1, 1), (0, 0, 1), (0, 0, 0)]


# ---- the camera ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("up_axis", [0, 1, 2])
def test_ray_directions_lie_in_the_field_of_view(up_axis):
    fwd, left = [a for a in range(3) if a != up_axis]
    hfov, vfov = 90.0, 60.0
    for yaw, pitch in ((0.0, 0.0), (0.7, 0.0), (math.pi, 0.2), (-2.0, -0.4), (math.pi / 2, 0.0)):
        d = view.ray_directions(hfov, vfov, 9, 5, yaw, pitch, up_axis)
        assert d.dtype == np.int32 and d.shape == (45, 3)
        assert np.abs(d).max(axis=1).tolist() == [view.MAX_DIR] * 45            # scaled to the largest component
        v = d.astype(np.float64)
        vf, vl, vu = v[:, fwd], v[:, left], v[:, up_axis]
        vf, vl = vf * math.cos(yaw) + vl * math.sin(yaw), -vf * math.sin(yaw) + vl * math.cos(yaw)      # undo the yaw
        vf, vu = vf * math.cos(pitch) + vu * math.sin(pitch), -vf * math.sin(pitch) + vu * math.cos(pitch)
        assert (vf > 0).all()
        tol = 1e-4                                                              # rounding to 1 / 32767
        assert (np.abs(vl / vf) <= math.tan(math.radians(hfov) / 2) + tol).all()
        assert (np.abs(vu / vf) <= math.tan(math.radians(vfov) / 2) + tol).all()
        # pixel centres: the outermost rays sit half a pixel inside the edge
        assert abs(np.abs(vl / vf).max() - math.tan(math.radians(hfov) / 2) * 8 / 9) < tol
        centre = d[len(d) // 2].astype(np.float64)                              # odd sizes: the heading itself
        want = np.zeros(3)
        want[fwd], want[left], want[up_axis] = (math.cos(pitch) * math.cos(yaw), math.cos(pitch) * math.sin(yaw),
                                                math.sin(pitch))
        assert np.abs(centre / np.linalg.norm(centre) - want).max() < 1e-4
    d = view.ray_directions(90.0, 60.0, 3, 1, 0.0, 0.0, up_axis)
    assert d[1].tolist() == [view.MAX_DIR if a == fwd else 0 for a in range(3)]   # yaw 0 looks along the lower axis
    assert d[2][left] > 0 > d[0][left]                                          # the image's x grows toward the higher
    d = view.ray_directions(90.0, 60.0, 1, 1, math.pi / 2, 0.0, up_axis)
    assert d[0].tolist() == [view.MAX_DIR if a == left else 0 for a in range(3)]  # positive yaw: toward the higher one
    assert (view.ray_directions(120.0, 60.0, 7, 1, 1.1, 0.0, 0)[:, 0] == 0).all()  # a map's row of rays has d_0 = 0


# ---- the choice ---------------------------------------------------------------------------------------------------------
def test_choose_applies_the_thresholds_the_decay_and_every_tie():
    #                heading 0          heading 1
    table = [[(5, 9, 2, 16), (9, 1, 0, 10)],        # view 0, cost 4000
             [(9, 3, 1, 13), (9, 3, 4, 16)],        # view 1, cost 2000
             [(9, 0, 3, 12), (2, 2, 2, 6)],         # view 2, cost 2000
             [(20, 0, 0, 20), (0, 5, 5, 10)]]       # view 3, cost 9000
    cost, lin, voxel = [4000, 2000, 2000, 9000], [70, 50, 30, 10], 0.5
    pick, n = view.choose(table, cost, lin, voxel)
    assert pick == (3, 0, 20 * 0.125) and n == 7                 # unknown >= 1: all but (3, 1)
    pick, n = view.choose(table, cost, lin, voxel, min_gain_cells=0)
    assert pick[:2] == (3, 0) and n == 8
    pick, n = view.choose(table, cost, lin, voxel, min_solid_cells=1)
    assert pick == (2, 0, 9 * 0.125) and n == 5                  # 9 three times at cost 2000: the lower linear index
    pick, n = view.choose(table, cost, [70, 30, 50, 10], voxel, min_solid_cells=1)
    assert pick[:2] == (1, 0) and n == 5                         # and within one view the lower heading
    pick, n = view.choose(table, [4000, 2000, 1999, 9000], lin, voxel, min_solid_cells=4)
    assert pick[:2] == (1, 1) and n == 1
    pick, n = view.choose(table[:3], [1000, 2000, 2000], lin[:3], voxel, min_gain_cells=6)
    assert pick[:2] == (0, 1) and n == 4                         # 9 four times: the lower cost
    pick, n = view.choose([[(9, 0, 0, 9)], [(9, 0, 0, 9)]], [3000, 1000], [1, 2], voxel)
    assert pick[:2] == (1, 0)                                    # equal scores: the lower cost
    # lam: 20 cells 4.5 m away against 9 cells 1 m away
    pick, _ = view.choose(table, cost, lin, voxel, lam=0.1)
    assert pick[:2] == (3, 0) and pick[2] == 20 * 0.125 * math.exp(-0.1 * 4.5)
    pick, _ = view.choose(table, cost, lin, voxel, lam=1.0)
    assert pick[:2] == (2, 0) and pick[2] == 9 * 0.125 * math.exp(-1.0)
    assert view.choose(table, cost, lin, voxel, min_gain_cells=21) == (None, 0)
    assert view.choose([], [], [], voxel) == (None, 0)


# ---- text ---------------------------------------------------------------------------------------------------------------
def test_parse_next_view_inverts_the_writer_bit_for_bit():
    rng = np.random.default_rng(5)
    found = {"view_cell": [3, 0, 1023], "view_point": [float(v) for v in rng.normal(size=3) * 7.3], "yaw": 2 * math.pi * 5 / 7,
             "yaw_index": 5, "gain_cells": 123456, "gain_m3": 123456 * 0.05 ** 3, "free_cells": 7, "solid_cells": 0,
             "score": 123456 * 0.05 ** 3 * math.exp(-0.3 * 1.7), "length_m": 1.7 / 3, "n_candidates": 4096,
             "n_qualified": 31, "gains": None, "cells": None}
    text = view.next_view_text(found)
    back = view.parse_next_view(text)
    assert back == {**{k: found[k] for k in view.REPORT_ORDER if k != "found"}, "found": True}
    assert view.next_view_text(back) == text
    on_map = dict(found, view_cell=(4, 9), view_point=[0.1 + 0.2, -1e-17])
    assert view.parse_next_view(view.next_view_text(on_map))["view_point"] == [0.1 + 0.2, -1e-17]
    nothing = dict(view._nothing(17, None), length_m=math.inf)
    back = view.parse_next_view(view.next_view_text(nothing))
    assert back["found"] is False and back["view_cell"] is None and back["yaw"] is None and back["length_m"] == math.inf
    assert back["n_candidates"] == 17 and back["gain_m3"] == 0.0 and back["yaw_index"] is None
    for bad in ("", "Frontiers of\n", text.replace("yaw_index", "heading"), text + "x\t1\n"):
        with pytest.raises(ValueError):
            view.parse_next_view(bad)


# ---- refusals that need no GPU ------------------------------------------------------------------------------------------
def stub_esdf(state):
    state = torch.from_numpy(np.ascontiguousarray(state))
    dims = tuple(state.shape)
    return tsdf.ESDF(state, torch.full(dims, 9, dtype=torch.int32), torch.full(dims, 0.3), [0.0, 0.0, 0.0], 0.1, dims, 3)


def test_view_gain_refuses_before_the_device_is_touched(monkeypatch):
    from go_slam_amd import _lib
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was reached"))
    ok = torch.ones(2, 3, 4, dtype=torch.uint8)
    o, d = [(0, 0, 0)], [(1, 2, 3)]
    for state in (ok.float(), ok.bool(), ok.numpy()):
        with pytest.raises(ValueError, match="state must be a uint8"):
            view.view_gain(state, o, d, 3)
    for state in (ok[0], torch.ones(1, 1, 1025, dtype=torch.uint8), torch.ones(0, 2, 2, dtype=torch.uint8)):
        with pytest.raises(ValueError, match=r"\[n0,n1,n2\]"):
            view.view_gain(state, o, d, 3)
    for origins in ([(0, 0)], [(0.5, 0, 0)], torch.zeros(1, 3, dtype=torch.int64), torch.zeros(3, dtype=torch.int32),
                    [(1 << 31, 0, 0)]):
        with pytest.raises(ValueError, match="origin"):
            view.view_gain(ok, origins, d, 3)
    for dirs in ([(1, 2)], [(0.5, 0, 0)], np.zeros((0, 3), dtype=np.int32), np.zeros((65537, 3), dtype=np.int32),
                 [(1, 2, 3, 4)]):
        with pytest.raises(ValueError, match="dirs must be|rays"):
            view.view_gain(ok, o, dirs, 3)
    for dirs in ([(32768, 0, 0)], [(0, -32768, 1)], torch.tensor([[1 << 40, 0, 0]])):
        with pytest.raises(ValueError, match="component outside"):
            view.view_gain(ok, o, dirs, 3)
    for r in (0, -1, 1772, 2.0, True):
        with pytest.raises(ValueError, match="range_cells"):
            view.view_gain(ok, o, d, r)
    for m in (-1, 1.0, False):
        with pytest.raises(ValueError, match="max_unknown"):
            view.view_gain(ok, o, d, 3, max_unknown=m)
    for box in ((0, 0, 0, 1, 1), (1, 0, 0, 2, 2, 2), (0, 0, 0, 0, -1, 0), "abc", (0, 0, None, 1, 1, 1)):
        with pytest.raises(ValueError, match="box must be"):
            view.view_gain(ok, o, d, 3, box=box)
    with pytest.raises(ValueError, match="at most 1048576"):
        view.view_gain(ok, o, d, 3, box=(-64, -64, -64, 63, 63, 64))
    # all six axes reach range + 2 cells: 101^3 = 1030301 cells fit, 103^3 do not, so range 48 is the largest
    axes = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    with pytest.raises(ValueError, match="largest range that fits is 48 cells"):
        view.view_gain(ok, o, axes, 60)
    assert view.gain_arguments(ok, o, axes, 48)[5] == (-50,) * 3 + (50,) * 3
    assert view.gain_arguments(ok, torch.zeros(0, 3, dtype=torch.int32), d, 1771, 5, (0, 0, 0, 0, 0, 0))[3:] == (
        1771, 5, (0, 0, 0, 0, 0, 0))
    assert view.MAX_RANGE ** 2 <= 3 * 1023 ** 2 < (view.MAX_RANGE + 1) ** 2


CAMERA = {"hfov_deg": 90.0, "vfov_deg": 60.0, "n_u": 8, "n_v": 6, "range_m": 1.0, "pitch_deg": 0.0}


def test_next_view_refuses_before_the_device_is_touched(monkeypatch):
    from go_slam_amd import _lib
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was reached"))
    field = stub_esdf(np.ones((4, 5, 6), dtype=np.uint8))
    args = ([0, 0, 0], CAMERA, 1, (0.0, 0.2))
    for camera in (None, {}, dict(CAMERA, hfov_deg=180.0), dict(CAMERA, vfov_deg=0.0), dict(CAMERA, range_m=0.0),
                   dict(CAMERA, n_u=0), dict(CAMERA, n_u=512, n_v=129), dict(CAMERA, fov=3), dict(CAMERA, n_v=1.5),
                   dict(CAMERA, pitch_deg=math.nan), dict(CAMERA, range_m="far")):
        with pytest.raises(ValueError, match="camera"):
            field.next_view([0, 0, 0], camera, 1, (0.0, 0.2))
    for range_m in (0.09, 178.0):                               # below one cell, beyond 1771 cells
        with pytest.raises(ValueError, match="range_m"):
            field.next_view([0, 0, 0], dict(CAMERA, range_m=range_m), 1, (0.0, 0.2))
    with pytest.raises(ValueError, match="largest range that fits is"):
        field.next_view([0, 0, 0], dict(CAMERA, hfov_deg=170.0, vfov_deg=170.0, range_m=30.0), 1, (0.0, 0.2))
    for key, values in (("n_yaw", (0, 1.5, True)), ("min_gain_cells", (-1, 0.5)), ("min_solid_cells", (-1, None)),
                        ("lam", (-0.1, math.inf, math.nan)), ("max_unknown", (-1, 2.5)), ("stride", (0, 1.0)),
                        ("max_candidates", (0, 7.5)), ("robot_radius", (-0.1, 0.31)), ("snap", (-1.0, math.inf)),
                        ("max_cost_m", (0.0, 1e9))):
        for v in values:
            with pytest.raises(ValueError, match=key):
                field.next_view(*args, **{key: v})
    for up_axis in (3, -1, 1.0):
        with pytest.raises(ValueError, match="up_axis"):
            field.next_view([0, 0, 0], CAMERA, up_axis, (0.0, 0.2))
    with pytest.raises(ValueError, match="no lattice layer"):
        field.next_view([0, 0, 0], CAMERA, 1, (0.01, 0.09))
    with pytest.raises(ValueError, match="three finite"):
        field.next_view([0, 0], CAMERA, 1, (0.0, 0.2))
    with pytest.raises(ValueError, match="outside the lattice"):
        field.view_candidates([0.36, 0, 0], 1, (0.0, 0.2))
    for key, v in (("stride", 0), ("max_candidates", 0), ("robot_radius", 0.31)):
        with pytest.raises(ValueError, match=key):
            field.view_candidates([0, 0, 0], 1, (0.0, 0.2), **{key: v})
    grid = {"cells": np.full((4, 5), 254, dtype=np.uint8), "origin": (-1.0, 2.0), "resolution": 0.5}
    with pytest.raises(ValueError, match="outside the map"):
        view.next_view_on_map(grid, (-1.01, 2.0), CAMERA)
    with pytest.raises(ValueError, match="camera"):
        view.next_view_on_map(grid, (0.0, 3.0), dict(CAMERA, hfov_deg=0.0))
    with pytest.raises(ValueError, match="range_m"):
        view.next_view_on_map(grid, (0.0, 3.0), dict(CAMERA, range_m=0.4))
    with pytest.raises(ValueError, match="n_yaw"):
        view.next_view_on_map(grid, (0.0, 3.0), CAMERA, n_yaw=0)
    with pytest.raises(ValueError, match="uint8"):
        view.next_view_on_map(dict(grid, cells=np.zeros((4, 5))), (0.0, 3.0), CAMERA)


# ---- the kernel's resources (compile-only) ------------------------------------------------------------------------------
@pytest.mark.parametrize("defines", [(), ("-DVIEW_READ_FIRST=1",), ("-DVIEW_PACKED=1",)], ids=lambda d: "".join(d) or "shipped")
def test_kernel_resources(tmp_path, defines):
    """csrc/view_gain.hip, the shipped form and the two measurement builds: no scratch, no static LDS in front of the
    dynamic mask, and at most 64 VGPRs, so that registers never stand between a small box and eight waves per SIMD; no
    floating-point and no global atomic instruction in the walk."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "go_slam_amd", "csrc")
    out = tmp_path / "k.s"
    res = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                          "-fno-gpu-rdc", "-munsafe-fp-atomics", "-I", csrc, "-I", os.path.join(ROOT, "include"), *defines,
                          "--cuda-device-only", "-S", os.path.join(csrc, "view_gain.hip"), "-o", str(out)],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-2000:]
    asm = open(out).read()
    pat = re.compile(r"\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.name:\s+(\S+)\n(?:.*\n)*?"
                     r"\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)")
    seen = []
    for m in pat.finditer(asm):
        lds, name, scratch, vgpr = int(m.group(1)), m.group(2), int(m.group(3)), int(m.group(4))
        print(name, "VGPRs", vgpr, "LDS", lds, "scratch", scratch)
        assert scratch == 0 and lds == 0 and vgpr <= 64, f"{name}: {scratch} B of scratch, {lds} B of LDS, {vgpr} VGPRs"
        seen.append(name)
    assert sum("view_gain_kernel" in n for n in seen) == 1 and len(seen) == (2 if "-DVIEW_PACKED=1" in defines else 1)
    body = asm[asm.index("view_gain_kernel"):]
    assert "ds_or_rtn_b32" in body                                # the returning LDS atomic
    assert not re.search(r"\b(global|flat|buffer)_atomic", body) and not re.search(r"\bv_\w*_f(16|32|64)\w*", body)
