"""`fuse_from_config`'s checks before the fusion, with every cfg["tsdf"] key on at once (go_slam_amd/tsdf_run.py): good
values reach the fusion and write nothing, of two bad keys the earlier one of the check order is reported, and a
switched-off key is not looked at.  No GPU and no library: the namespace has no `video`, so reaching the fusion is an
AttributeError."""
import copy
import os
import sys
import types

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from go_slam_amd import tsdf                                   # noqa: E402
import test_tsdf_merge_cpu as MC                               # noqa: E402

UP = [0.0, -1.0, 0.0]


@pytest.fixture
def every_key(tmp_path):
    """cfg["tsdf"] with every key on and good values; merge reads a volume saved on the host."""
    MC.host_volume().save(str(tmp_path / "earlier.npz"))
    plan = {"enable": True, "robot_radius": 0.2, "snap": 1.0, "allow_unknown": True, "goal": [0.6, 0.0, 0.3],
            "straighten": {"enable": True, "window": 128},
            "follow": {"enable": True, "up_axis": 1, "K": 256, "max_ticks": 80}}
    camera = {"hfov_deg": 90.0, "vfov_deg": 60.0, "n_u": 16, "n_v": 12, "range_m": 2.0, "pitch_deg": 0.0}
    esdf = {"enable": True, "max_distance": 1.0, "save_volume": True,
            "slice": {"up_axis": 1, "height": [-0.5, 0.5], "robot_radius": 0.2}, "plan": plan,
            "frontiers": {"enable": True, "robot_radius": 0.2, "snap": 1.0, "min_cells": 2},
            "next_view": {"enable": True, "camera": camera, "up_axis": 1, "height": [-0.5, 0.5], "n_yaw": 4},
            "rooms": {"enable": True, "robot_radius": 0.2, "core_radius": 0.6},
            "floor": {"enable": True, "up_axis": 2, "height": [-0.1, 0.3], "robot_radius": 0.15, "robot_height": 0.3,
                      "step_height": 0.05, "plan": True},
            "scan": {"up_axis": 2, "height": [3.0, 3.6], "beams": 48, "fov_deg": 270.0, "max_range": 3.0, "every": 2,
                     "n_yaw": 24, "window_m": 0.5}}
    return {"enable": True, "voxel_size": 0.1, "bound": [[-1, 1]] * 3, "save_volume": True,
            "merge": {"enable": True, "volume": str(tmp_path / "earlier.npz"), "init": np.eye(4).tolist()},
            "align": {"enable": True, "every": 3}, "planes": {"enable": True, "min_cells": 100},
            "upright": {"enable": True, "up_hint": UP}, "objects": {"enable": True, "min_cells": 4},
            "eval_depth": {"enable": True, "every": 5}, "esdf": esdf}


def run(tsdf_cfg, out, stream=()):
    slam = types.SimpleNamespace(cfg={"mode": "rgbd", "tsdf": tsdf_cfg}, output=str(out), mode="rgbd")
    return tsdf.fuse_from_config(slam, stream=stream, c2w_list=[], stats={})


def put(cfg, path, value):
    """A deep copy of `cfg` with the value at the dotted `path` replaced."""
    cfg = copy.deepcopy(cfg)
    *parents, last = path.split(".")
    at = cfg
    for name in parents:
        at = at[name]
    at[last] = value
    return cfg


def test_every_key_on_with_good_values_reaches_the_fusion_and_writes_nothing(every_key, tmp_path):
    with pytest.raises(AttributeError, match="video"):
        run(every_key, tmp_path / "out")
    assert not os.path.exists(tmp_path / "out")


# one bad value per key, in the order the keys are checked: (what the refusal names, path, value)
BAD = {"merge": ("tsdf.merge.init", "merge.init", [[1, 0, 0], [0, 1, 0]]),
       "align": ("tsdf.align needs the stream", None, None),                      # the stream is an argument, no key
       "up_hint": ("tsdf.upright.up_hint", "upright.up_hint", "sideways"),
       "heading": ("tsdf.upright.heading", "upright.heading", "north"),
       "objects": ("tsdf.objects: min_cells", "objects.min_cells", 0),
       "rooms": ("tsdf.esdf.rooms", "esdf.rooms.core_radius", "wide"),
       "straighten": ("tsdf.esdf.plan.straighten", "esdf.plan.straighten", "yes"),
       "follow": ("tsdf.esdf.plan.follow", "esdf.plan.follow.K", -1),
       "floor": ("tsdf.esdf.floor", "esdf.floor.robot_radius", 0.1),
       "floor_plan": ("tsdf.esdf.floor.plan replans", "esdf.plan.enable", False),
       "scan": ("tsdf.esdf.scan", "esdf.scan.beams", 0)}
ORDER = list(BAD)


def spoiled(cfg, names):
    stream = ()
    for name in names:
        if BAD[name][1] is None:
            stream = None
        else:
            cfg = put(cfg, BAD[name][1], BAD[name][2])
    return cfg, stream


@pytest.mark.parametrize("name", ORDER)
def test_each_bad_value_is_refused_before_anything_is_fused(every_key, tmp_path, name):
    with pytest.raises(ValueError, match="fuse_from_config: " + BAD[name][0]):
        cfg, stream = spoiled(every_key, [name])
        run(cfg, tmp_path / "out", stream)
    assert not os.path.exists(tmp_path / "out")


@pytest.mark.parametrize("first, second", [("rooms", "scan"), ("merge", "align"), ("objects", "floor"),
                                           ("straighten", "follow")] + list(zip(ORDER, ORDER[1:])))
def test_of_two_bad_keys_the_earlier_one_is_reported(every_key, tmp_path, first, second):
    assert ORDER.index(first) < ORDER.index(second)
    cfg, stream = spoiled(every_key, [second, first])
    with pytest.raises(ValueError, match="fuse_from_config: " + BAD[first][0]):
        run(cfg, tmp_path / "out", stream)
    assert not os.path.exists(tmp_path / "out")


OFF = [("merge", {"enable": False, "volume": "nothing.npz", "init": "none"}, {}),
       ("align", {"enable": False, "every": "often"}, {"stream": None}),
       ("planes", {"enable": False, "bins": "many"}, {}),
       ("upright", {"enable": False, "up_hint": UP, "max_tilt_deg": "steep", "up_axis": 7}, {}),  # the objects' hint too
       ("objects", {"enable": False, "min_cells": 0, "min_area_m2": -1.0}, {}),
       ("eval_depth", {"enable": False, "every": 0}, {}),
       ("esdf", {"enable": False, "max_distance": "far", "rooms": {"enable": True, "core_radius": "wide"},
                 "plan": {"enable": True, "straighten": "yes"}, "floor": True, "scan": {"beams": 0}}, {}),
       ("esdf.plan", {"enable": False, "straighten": "yes", "follow": "closely", "start": "nowhere"},
        {"esdf.floor.plan": False}),
       ("esdf.plan.follow", {"enable": False, "K": -1}, {}),
       ("esdf.frontiers", {"enable": False, "start": "nowhere", "order": 3}, {}),
       ("esdf.next_view", {"enable": False, "start": "nowhere"}, {}),
       ("esdf.rooms", {"enable": False, "core_radius": "wide", "speed": 1.0}, {}),
       ("esdf.floor", {"enable": False, "robot_radius": "wide"}, {}),
       ("esdf.scan", {"enable": False, "beams": 0}, {})]


@pytest.mark.parametrize("key, value, also", OFF, ids=[o[0] for o in OFF])
def test_a_switched_off_key_is_not_looked_at(every_key, tmp_path, key, value, also):
    cfg = put(every_key, key, value)
    stream = ()
    for path, v in also.items():
        if path == "stream":
            stream = v
        else:
            cfg = put(cfg, path, v)
    with pytest.raises(AttributeError, match="video"):
        run(cfg, tmp_path / "out", stream)
    assert not os.path.exists(tmp_path / "out")


def test_a_straightening_window_is_checked_even_when_switched_off(every_key, tmp_path):
    with pytest.raises(ValueError, match="fuse_from_config: tsdf.esdf.plan.straighten"):
        run(put(every_key, "esdf.plan.straighten", {"enable": False, "window": "wide"}), tmp_path / "out")
    assert not os.path.exists(tmp_path / "out")
