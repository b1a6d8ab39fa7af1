"""One whole only-tracking run with every cfg["tsdf"] key on at once (go_slam_amd/tsdf_run.py), on the MI355X: the files it
writes and the statistics it returns are the ones listed here, every text file reads back and writes itself again byte
for byte, and the keys that read each other's products do: the rooms file lists the rooms along the planned route and
the room of every object in the map frame, the floor route is planned between the route's end cells, the objects file
has its map-frame block.  tsdf.merge is covered by a second call on the same run's video, and a third one plans the
floor route without `upright`, in the frame the floor key's own values were chosen for."""
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import test_tsdf_gpu as TG                                     # noqa: E402

pytestmark = pytest.mark.gpu

BASE = {"enable": True, "source": "sensor", "voxel_size": 0.1}


def every_key_cfg():
    """Each key with the values of its own whole-run test."""
    plan = {"enable": True, "robot_radius": 0.2, "snap": 1.0, "allow_unknown": True, "goal": [0.6, 0.0, 0.3],
            "straighten": {"enable": True, "window": 128},
            "follow": {"enable": True, "up_axis": 1, "K": 256, "max_ticks": 80}}
    camera = {"hfov_deg": 90.0, "vfov_deg": 60.0, "n_u": 16, "n_v": 12, "range_m": 2.0, "pitch_deg": 0.0}
    esdf = {"enable": True, "max_distance": 1.0, "save_volume": True,
            "slice": {"up_axis": 1, "height": [-0.5, 0.5], "robot_radius": 0.2}, "plan": plan,
            "frontiers": {"enable": True, "robot_radius": 0.2, "snap": 1.0, "min_cells": 2},
            "next_view": {"enable": True, "camera": camera, "up_axis": 1, "height": [-0.5, 0.5], "n_yaw": 4,
                          "robot_radius": 0.2, "stride": 2, "snap": 1.0, "min_gain_cells": 2},
            "rooms": {"enable": True, "robot_radius": 0.2, "core_radius": 0.4, "min_core_m3": 0.002, "snap": 1.0},
            "floor": {"enable": True, "up_axis": 1, "up_sign": -1, "height": [-3.0, 2.0], "robot_radius": 0.15,
                      "robot_height": 0.3, "step_height": 0.1, "plan": True},
            "scan": {"up_axis": 2, "height": [3.0, 3.6], "beams": 48, "fov_deg": 270.0, "max_range": 3.0, "every": 2,
                     "n_yaw": 24, "window_m": 0.5}}
    return dict(BASE, save_volume=True, planes={"enable": True, "min_cells": 100},
                upright={"enable": True, "up_hint": "camera"}, objects={"enable": True, "min_cells": 4},
                eval_depth={"enable": True, "every": 5}, align={"enable": True, "every": 3, "min_count": 32}, esdf=esdf)


def run_every_key(root):
    """The run with every key into {root}/run, then `fuse_from_config` on the same video twice more: with tsdf.merge
    into {root}/merge, joining the run's volume with its own saved one, and with esdf.plan and esdf.floor alone,
    between two points above the floor the volume holds, into {root}/floor.  -> the statistics of the run and of the
    two calls."""
    from go_slam_amd.slam import SLAM
    from go_slam_amd.tsdf import fuse_from_config
    returned = []
    terminate = SLAM.terminate

    def keeping(self, *args, **kw):
        returned.append(terminate(self, *args, **kw))
        return returned[-1]
    SLAM.terminate = keeping
    try:
        slam = TG.whole_run(f"{root}/run", every_key_cfg())
    finally:
        SLAM.terminate = terminate
    slam.output = f"{root}/merge"
    slam.cfg["tsdf"] = dict(BASE, merge={"enable": True, "volume": f"{root}/run/mesh/tsdf_volume.npz", "register": False,
                                         "init": np.eye(4).tolist()})
    poses = torch.from_numpy(np.load(f"{root}/run/checkpoints/est_poses.npy"))
    merge_stats, floor_stats = {}, {}
    fuse_from_config(slam, c2w_list=poses, stats=merge_stats)
    # the floor this volume holds is a strip before the wall z = 4, at y = 1.15, x from -1.7 to 1.6 and z from 3.4 to
    # 3.7: a route half a metre above it, from one lattice point over the strip to another, with no snapping
    slam.output = f"{root}/floor"
    slam.cfg["tsdf"] = dict(BASE, esdf={"enable": True, "max_distance": 1.0, "floor": every_key_cfg()["esdf"]["floor"],
                                        "plan": {"enable": True, "robot_radius": 0.2, "allow_unknown": True,
                                                 "start": [-1.0, 0.7, 3.5], "goal": [1.0, 0.7, 3.5]}})
    fuse_from_config(slam, c2w_list=poses, stats=floor_stats)
    torch.cuda.synchronize()
    return returned[0], merge_stats, floor_stats


def written_again(name, text):
    """The text file `name` of a run parsed and serialised again by its own pair of functions."""
    from go_slam_amd import (floor, follow, frontier, localize, plan, rooms, scan, tsdf, tsdf_merge, tsdf_objects,
                             tsdf_planes, view)
    if name == "metrics_tsdf_planes.txt":
        planes, at = tsdf_planes.parse_planes(text)
        return tsdf_planes.planes_text(planes, None if at is None else planes[at])
    if name == "metrics_tsdf_depth.txt":
        result, frames = tsdf.parse_depth_metrics(text)
        return tsdf.depth_metrics_text(result, [f[0] for f in frames], [list(f[1:]) + [0] for f in frames])
    if name == "metrics_tsdf_align.txt":
        _, frames = localize.parse_align(text)
        rows = np.array([f[1:] for f in frames], np.float64)
        return localize.align_text(localize.summarize_align(rows), [f[0] for f in frames], rows)
    if name == "map/path_straight.txt":
        head, points = plan.parse_straight_path(text)
        return plan.straight_path_text({"reachable": head["reachable"], "straight_length_m": head["length_m"],
                                        "straight_min_clearance_m": head["min_clearance_m"], "waypoint_points": points,
                                        "length_m": head["lattice_length_m"],
                                        "cells": np.zeros((head["n_lattice_points"], 3))})
    if name == "map/follow.txt":
        head, trace, controls = follow.parse_follow(text)
        return follow.follow_text(dict(head, trace=trace, controls=controls))
    if name.endswith("path.txt"):
        head, points = plan.parse_path(text)
        return plan.path_text(dict(head, points=points))
    simple = {"metrics_tsdf_clearance.txt": lambda t: tsdf.clearance_text(tsdf.parse_clearance(t)),
              "metrics_tsdf_merge.txt": lambda t: tsdf_merge.merge_text(*tsdf_merge.parse_merge(t)),
              "map/upright.txt": lambda t: tsdf_planes.transform_text(tsdf_planes.parse_transform(t)),
              "map/objects.txt": lambda t: tsdf_objects.objects_text(*tsdf_objects.parse_objects(t)),
              "map/frontiers.txt": lambda t: frontier.frontiers_text(frontier.parse_frontiers(t)),
              "map/next_view.txt": lambda t: view.next_view_text(view.parse_next_view(t)),
              "map/rooms.txt": lambda t: rooms.rooms_text(rooms.parse_rooms(t)),
              "map/floor.txt": lambda t: floor.floor_text(floor.parse_floor(t)),
              "map/scan_localize.txt": lambda t: scan.scan_localize_text(scan.parse_scan_localize(t))}
    return simple[name](text)


RUN_FILES = ["checkpoints/est_poses.npy", "checkpoints/go.ckpt", "map/explore_path.txt", "map/floor.txt",
             "map/floor/occupancy.pgm", "map/floor/occupancy.yaml", "map/floor_path.txt", "map/follow.txt",
             "map/frontiers.txt", "map/next_view.txt", "map/next_view_path.txt", "map/objects.txt", "map/occupancy.pgm",
             "map/occupancy.yaml", "map/path.txt", "map/path_straight.txt", "map/rooms.txt", "map/scan_localize.txt",
             "map/upright.txt",
             "mesh/tsdf_esdf.npz", "mesh/tsdf_mesh.ply", "mesh/tsdf_volume.npz", "metrics_traj.txt",
             "metrics_tsdf_align.txt", "metrics_tsdf_clearance.txt", "metrics_tsdf_depth.txt", "metrics_tsdf_planes.txt"]
MERGE_FILES = ["mesh/tsdf_merged_mesh.ply", "mesh/tsdf_mesh.ply", "metrics_tsdf_merge.txt"]
RUN_STATS = {"tsdf_align_failed", "tsdf_align_moved_constrained_mean_m", "tsdf_align_moved_max_m",
             "tsdf_align_moved_mean_m",
             "tsdf_clearance_inside", "tsdf_clearance_min_m", "tsdf_clearance_unknown", "tsdf_coverage", "tsdf_depth_l1_cm",
             "tsdf_doors_found", "tsdf_explore_reachable", "tsdf_floor_found", "tsdf_floor_map_drivable_m2",
             "tsdf_floor_map_unknown_m2", "tsdf_floor_path_length_m", "tsdf_floor_path_reachable",
             "tsdf_follow_min_clearance_m", "tsdf_follow_reached", "tsdf_follow_ticks", "tsdf_frontier_cells",
             "tsdf_frontier_clusters", "tsdf_n_frames", "tsdf_next_view_candidates", "tsdf_next_view_found",
             "tsdf_next_view_gain_m3", "tsdf_objects_found", "tsdf_objects_on_floor", "tsdf_path_length_m",
             "tsdf_path_reachable", "tsdf_path_straight_length_m", "tsdf_path_waypoints", "tsdf_planes_found",
             "tsdf_rooms_found", "tsdf_scan_poses_recovered", "tsdf_scan_poses_tried", "tsdf_unknown_fraction"}
MERGE_STATS = {"tsdf_merge_overlap", "tsdf_merge_rmse_m", "tsdf_merge_moved_m", "tsdf_merge_ok"}
NOT_TSDF_TEXT = {"metrics_traj.txt"}                           # terminate's own
FLOOR_UP_AXIS = 1                                              # every_key_cfg()'s esdf.floor.up_axis
FLOOR_ROUTE = {"run": False, "floor": True}                    # tsdf_floor_path_reachable of the two seeded calls


def test_a_run_with_every_key_writes_every_file(built_lib, tmp_path):
    from go_slam_amd import plan, rooms, tsdf, tsdf_merge, tsdf_objects, tsdf_planes
    stats, merge_stats, floor_stats = run_every_key(str(tmp_path))
    out, out2, out3 = (str(tmp_path / name) for name in ("run", "merge", "floor"))
    assert [p.replace(os.sep, "/") for p in TG.listing(out)] == RUN_FILES
    assert [p.replace(os.sep, "/") for p in TG.listing(out2)] == MERGE_FILES
    assert {k for k in stats if k.startswith("tsdf_")} == RUN_STATS
    assert set(merge_stats) == MERGE_STATS
    for root, names in ((out, RUN_FILES), (out2, MERGE_FILES)):
        for name in names:
            if name.endswith(".txt") and name not in NOT_TSDF_TEXT:
                text = open(f"{root}/{name}").read()
                assert written_again(name, text) == text, name
    for directory in ("map", "map/floor"):                     # the two map_server maps
        tsdf.save_map(str(tmp_path / "again" / directory), tsdf.load_map(f"{out}/{directory}"))
        for name in ("occupancy.pgm", "occupancy.yaml"):
            assert open(tmp_path / "again" / directory / name, "rb").read() == open(f"{out}/{directory}/{name}", "rb").read()

    # objects: a second block, the first one moved by map/upright.txt
    boxes, moved = tsdf_objects.parse_objects(open(f"{out}/map/objects.txt").read())
    T = tsdf_planes.parse_transform(open(f"{out}/map/upright.txt").read())
    assert moved is not None and len(moved) == len(boxes) == stats["tsdf_objects_found"]
    for b, m in zip(boxes, moved):
        assert np.abs(m["centre"] - (T[:3, :3] @ b["centre"] + T[:3, 3])).max() < 1e-12
    # rooms: the route's rooms when it is reachable, and the room of every object, looked up in the map frame: the open
    # cell it was taken from lies within the object's largest half extent of the object's centre there
    report = rooms.parse_rooms(open(f"{out}/map/rooms.txt").read())
    head, _ = plan.parse_path(open(f"{out}/map/path.txt").read())
    print("rooms:", {k: report[k] for k in rooms.SUMMARY_ORDER}, "path:", head)
    assert head["reachable"] and stats["tsdf_path_reachable"]                      # in this run, as recorded
    assert report["along_rooms"] is not None and report["along_doors"] is not None
    assert report["object_rooms"] is not None and len(report["object_rooms"]) == len(moved)
    assert report["camera_room"] is not None
    for m, room in zip(moved, report["object_rooms"]):
        assert -1 <= room < report["n_rooms"]
        if room >= 0:
            lo, hi = (np.array([report["rooms"][f"{end}_{a}"][room] for a in "xyz"]) for end in ("lo", "hi"))
            reach = 0.5 * float(np.max(m["size_m"])) + 0.1
            assert (m["centre"] >= lo - reach).all() and (m["centre"] <= hi + reach).all()
    # floor.plan: map/floor_path.txt is written whenever it is on, and a floor route runs between the columns of the end
    # cells of map/path.txt: on the floor map's two axes it starts and ends where that route does, in that order.  In
    # the upright run the floor key's values, chosen for the run's own frame, leave no drivable column and no route
    for root, run_stats, reachable in ((out, stats, FLOOR_ROUTE["run"]), (out3, floor_stats, FLOOR_ROUTE["floor"])):
        floor_head, floor_points = plan.parse_path(open(f"{root}/map/floor_path.txt").read())
        head, points = plan.parse_path(open(f"{root}/map/path.txt").read())
        assert floor_head["reachable"] == run_stats["tsdf_floor_path_reachable"] == reachable and head["reachable"]
        assert floor_head["n_points"] == len(floor_points)
        assert floor_head["length_m"] == run_stats["tsdf_floor_path_length_m"]
        if reachable:
            axes = [a for a in range(3) if a != FLOOR_UP_AXIS]
            assert np.abs(floor_points[[0, -1]][:, axes] - points[[0, -1]][:, axes]).max() < 1e-6      # of a 0.1 m cell
            assert np.abs(points[0] - points[-1])[axes].max() > 1.0                # the two ends are two places
        else:
            assert len(floor_points) == 0 and floor_head["length_m"] == math.inf
    # merge: the second call joined the run's volume with its own saved one, as given
    result, T_merge = tsdf_merge.parse_merge(open(f"{out2}/metrics_tsdf_merge.txt").read())
    assert result["registered"] == 0 and np.array_equal(T_merge, np.eye(4)[:3])
    assert merge_stats["tsdf_merge_ok"] is True and math.isnan(merge_stats["tsdf_merge_overlap"])
    assert open(f"{out2}/mesh/tsdf_mesh.ply", "rb").read() == open(f"{out}/mesh/tsdf_mesh.ply", "rb").read()
