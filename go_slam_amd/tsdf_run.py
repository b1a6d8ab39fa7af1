"""`SLAM.terminate`'s TSDF step, `fuse_from_config`: one checked stage per cfg["tsdf"] key.

Every key has a `check_*` function that runs before anything is fused -- it returns the key's arguments, or None when
the key is off, and raises what the key refuses that early -- and one or two functions that take those arguments after
the fusion: first those that may still refuse (`join_merge`, `find_planes`, `stand_upright`, `find_objects`: before
anything is written), then the `write_*` ones in the order of the files.  `fuse_from_config` lists them in order and
skips the ones whose arguments are None.  A `check_*` docstring states its key's sub-keys, defaults, files, `stats`
names and refusals; DESIGN.md section 37 has them in one table.  `Run` carries what the stages share.
"""
import math
import os

import numpy as np
import torch

from . import floor as _floor
from . import follow as _follow
from . import frontier as _frontier
from . import localize as _localize
from . import plan as _plan
from . import rooms as _rooms
from . import scan as _scan
from . import mcl as _mcl
from . import tsdf as _tsdf
from . import tsdf_merge as _merge
from . import tsdf_objects as _objects
from . import tsdf_planes as _planes
from . import view as _view

WHAT = "fuse_from_config: tsdf"


def _on(opt):
    """The key's dict when it is switched on, else None."""
    opt = opt or {}
    return opt if opt.get("enable", False) else None


class Run:
    """What the stages of one `fuse_from_config` call share: the call's arguments, the `tsdf` options, and what the
    stages made so far -- `vol` and `mesh` (the fusion), `merged`, `planes`, `floor`, `upright` (None or the upright
    volume and the transform world to map), `objects`, `field` (the distance field) and `planned` (the route of
    esdf.plan).  The keys under `esdf` run on `nav_vol` with the poses `nav_c2w`: the run's own, or under `upright` the
    ones in the map frame."""

    def __init__(self, slam, opt, stream, trans_init, c2w_list, stats):
        self.slam, self.opt, self.stream, self.trans_init = slam, opt, stream, trans_init
        self.c2w_list, self.stats = c2w_list, stats
        self.esdf = _on(opt.get("esdf")) or {}                 # {} when off: none of its keys is looked at
        level = {k: opt.get(k) or {} for k in ("planes", "upright", "objects")}
        # with one of the three on the planes are found, with all three's values, and where up is matters
        self.level = level if any(o.get("enable", False) for o in level.values()) else None
        self.up_hint = self.min_weight = self.vol = self.mesh = self.merged = self.planes = self.floor = None
        self.upright = self.objects = self.field = self.planned = self.nav_vol = None
        self.nav_c2w = c2w_list

    @property
    def voxel_size(self):                                      # converted where it is used: a bad one is refused there
        return float(self.opt.get("voxel_size", 0.05))

    def path(self, relative_path):
        return f"{self.slam.output}/{relative_path}"

    def write(self, relative_path, text):
        os.makedirs(os.path.dirname(self.path(relative_path)), exist_ok=True)
        with open(self.path(relative_path), "w") as fh:
            fh.write(text)

    def report(self, values, *lines):
        """`values` into the caller's `stats`, when there are any, and the lines to the console."""
        if self.stats is not None:
            self.stats.update(values)
        for line in lines:
            print(line)

    def intrinsics(self):
        return (self.slam.video.intrinsics[0] * 8).cpu().tolist()

    def map_point(self, value):
        """A world point moved to the frame of `nav_vol`; a name ("last", "first") as it is."""
        return value if isinstance(value, str) or self.upright is None else _planes.moved_point(self.upright[1], value)

    def camera_point(self, value, key, allowed):
        """The start or goal `value` of esdf.`key` (after `map_point`) as a point: one of the names `allowed` ("last" /
        "first") is that camera centre of `nav_c2w`.  Refused late, after the files of the stages before: a name
        without a pose, and for a key that allows "last" alone any other name (esdf.plan hands one on to `ESDF.plan`)."""
        if not isinstance(value, str) or (value not in allowed and len(allowed) > 1):
            return value
        if value not in allowed:
            raise ValueError(f"{WHAT}.esdf.{key}.start is a world point or 'last' (got {value!r})")
        if len(self.c2w_list) == 0:
            raise ValueError(f"{WHAT}.esdf.{key} needs a camera pose for " + " / ".join(repr(a) for a in allowed))
        return torch.as_tensor(self.nav_c2w[-1 if value == "last" else 0])[:3, 3]


def check_merge(run):
    """tsdf.merge = {enable, volume, init, register, levels, huber, min_count, save_volume} (absent by default): the
    volume an earlier run saved at `volume` (TSDFVolume.save) is loaded, this run's volume is registered to it from
    `init` (a 4 x 4 list, this run's world to the earlier run's; absent: the identity; register false takes it as it
    is) and both are merged into a union volume in the earlier run's world (tsdf_merge.join_volumes).  Files:
    mesh/tsdf_merged_mesh.ply, metrics_tsdf_merge.txt (tsdf_merge.merge_text) and, with save_volume,
    mesh/tsdf_merged_volume.npz.  stats: tsdf_merge_overlap, tsdf_merge_rmse_m, tsdf_merge_moved_m, tsdf_merge_ok.
    Refuses before the fusion a missing or unreadable file and a bad `init`, and before anything is written (`join_merge`)
    a failed registration."""
    mg = _on(run.opt.get("merge"))
    if mg is None:
        return None
    path = mg.get("volume")
    if not path or not os.path.isfile(path):
        raise ValueError(f"{WHAT}.merge.volume {path!r} is no file (TSDFVolume.save writes one)")
    try:
        earlier = _tsdf.TSDFVolume.load(path, device="cpu")
    except Exception as e:
        raise ValueError(f"{WHAT}.merge.volume {path!r} cannot be read as a saved volume: {e}") from None
    init = _merge.transforms34(np.eye(4) if mg.get("init") is None else np.asarray(mg["init"], np.float64),
                               f"{WHAT}.merge.init")
    return mg, earlier, init


def join_merge(run, args):
    mg, earlier, init = args
    for name in ("tsdf", "weight", "colors"):
        setattr(earlier, name, getattr(earlier, name).to(run.vol.device))
    earlier.device = run.vol.device
    run.merged = _merge.join_volumes([earlier, run.vol], [None, init[0]], register=mg.get("register", True),
                                     min_weight=run.min_weight, levels=mg.get("levels", _merge.DEFAULT_LEVELS),
                                     huber=mg.get("huber", 0.5), min_count=mg.get("min_count", 64))


def write_merge(run, args):
    joined, transforms, reports = run.merged
    joined.extract_mesh(run.min_weight).export(run.path("mesh/tsdf_merged_mesh.ply"))
    res = _merge.merge_report(reports[1])
    run.write("metrics_tsdf_merge.txt", _merge.merge_text(res, transforms[1]))
    if args[0].get("save_volume", False):
        joined.save(run.path("mesh/tsdf_merged_volume.npz"))
    run.report(dict(tsdf_merge_overlap=res["overlap"], tsdf_merge_rmse_m=res["rmse_m"], tsdf_merge_moved_m=res["moved_m"],
                    tsdf_merge_ok=bool(res["ok"])),
               "TSDF merge: " + ", ".join(f"{k} {res[k]!r}" for k in _merge.MERGE_REPORT_ORDER))


def check_align(run):
    """tsdf.align = {enable, every 5, levels, huber 0.5, max_depth inf, min_count 64} (absent by default; rgbd mode
    only): every `every`-th frame of the stream is aligned to the run's own volume from its pose (localize.align_stream)
    into metrics_tsdf_align.txt (localize.align_text).  stats: tsdf_align_moved_mean_m, tsdf_align_moved_max_m,
    tsdf_align_moved_constrained_mean_m (along the directions the surfaces in view constrain), tsdf_align_failed.
    Refuses before the fusion another mode and a missing stream or pose list."""
    al = _on(run.opt.get("align"))
    if al is None:
        return None
    if run.slam.cfg.get("mode", "rgbd") != "rgbd":
        raise ValueError(f"{WHAT}.align needs rgbd mode (mode is {run.slam.cfg.get('mode')!r}: no sensor depth to align)")
    if run.stream is None or run.c2w_list is None:
        raise ValueError(f"{WHAT}.align needs the stream and its camera-to-world poses")
    return al


def write_align(run, al):
    res = _localize.align_stream(run.vol, run.stream, run.c2w_list, run.intrinsics(), every=al.get("every", 5),
                                 out_path=run.path("metrics_tsdf_align.txt"),
                                 levels=al.get("levels", _localize.DEFAULT_LEVELS), huber=al.get("huber", 0.5),
                                 max_depth=al.get("max_depth", math.inf), min_count=al.get("min_count", 64),
                                 min_weight=run.min_weight)
    run.report(dict(tsdf_align_moved_mean_m=res["moved_mean_m"], tsdf_align_moved_max_m=res["moved_max_m"],
                    tsdf_align_moved_constrained_mean_m=res["moved_constrained_mean_m"], tsdf_align_failed=res["n_failed"]),
               "TSDF align: " + ", ".join(f"{k} {res[k]!r}" for k in _localize.ALIGN_REPORT_ORDER))


def check_upright(run):
    """tsdf.upright = {enable, up_hint, max_tilt_deg 35, up_axis 2, up_sign 1, heading, save_volume} (absent by default;
    up_hint is a vector or "camera", minus the y column of the first pose, the default; heading absent or "walls"): the
    volume is stood upright on its floor (tsdf_planes.floor_plane, TSDFVolume.upright) and everything under `esdf` runs
    on the upright volume, in the map frame, with the poses and explicit points moved there; the mesh, objects,
    eval_depth, align and merge keep the run's own volume.  Files: map/upright.txt, the transform world to map
    (tsdf_planes.transform_text), and with save_volume mesh/tsdf_upright_volume.npz.  No stats.  up_hint and heading
    are looked at, and refused before the fusion, when any of planes, upright and objects is on ("camera" without poses
    only under upright itself); a volume without a floor is refused before anything is written (`stand_upright`)."""
    if run.level is None:
        return None
    up = run.level["upright"]
    hint = up.get("up_hint", "camera")
    if isinstance(hint, str):
        if hint != "camera":
            raise ValueError(f"{WHAT}.upright.up_hint is a vector or 'camera' (got {hint!r})")
        if run.c2w_list is not None and len(run.c2w_list) > 0:          # a camera's y axis points down
            hint = (-torch.as_tensor(run.c2w_list[0])[:3, 1]).double().tolist()
        elif up.get("enable", False):
            raise ValueError(f"{WHAT}.upright.up_hint 'camera' needs the run's camera-to-world poses")
        else:
            hint = None
    if hint is not None:
        run.up_hint = _planes._vector3(hint, f"{WHAT}.upright", "up_hint")
    if up.get("heading") not in (None, "walls"):
        raise ValueError(f"{WHAT}.upright.heading must be absent or 'walls' (got {up.get('heading')!r})")
    return _on(up)


def check_planes(run):
    """tsdf.planes = {enable, bins, cone_deg, band, max_planes, min_cells} (absent by default; TSDFVolume.find_planes'
    defaults): the fused volume's dominant planes and which of them is the floor under upright.up_hint go to
    metrics_tsdf_planes.txt (tsdf_planes.planes_text).  stats: tsdf_planes_found, tsdf_floor_found.  The planes are
    found with these values whenever one of planes, upright and objects is on; refuses nothing before the fusion."""
    return _on(run.opt.get("planes"))


def check_objects(run):
    """tsdf.objects = {enable, min_area_m2 2.0, cone_deg, band, min_cells} (absent by default): what stands on none of
    the structure planes (tsdf_objects.structure_planes, the floor first; TSDFVolume.find_objects on the run's own
    volume, up the floor's normal, or up_hint when there is no floor) goes to map/objects.txt in the run's world
    (tsdf_objects.objects_text), with `upright` a second block in the map frame.  stats: tsdf_objects_found,
    tsdf_objects_on_floor.  Refuses before the fusion a bad value and a run that cannot say where up is (no poses and
    no vector upright.up_hint)."""
    ob = _on(run.opt.get("objects"))
    if ob is None:
        return None
    find_args = {k: ob[k] for k in ("cone_deg", "band", "min_cells") if k in ob}
    if run.up_hint is None:
        raise ValueError(f"{WHAT}.objects needs to know where up is: the run's camera-to-world poses or a vector "
                         "tsdf.upright.up_hint")
    _objects.find_arguments(f"{WHAT}.objects", run.voxel_size, [], run.up_hint, **find_args)
    _objects.structure_planes([], None, ob.get("min_area_m2", 2.0))
    return ob, find_args


def find_planes(run, level):
    pc, up = level["planes"], level["upright"]
    run.planes = run.vol.find_planes(min_weight=run.min_weight, **{
        k: pc[k] for k in ("bins", "cone_deg", "band", "max_planes", "min_cells") if k in pc})
    if run.up_hint is not None:
        run.floor = _planes.floor_plane(run.planes, run.up_hint, up.get("max_tilt_deg", 35.0))


def stand_upright(run, up):
    if run.floor is None:
        raise ValueError(f"{WHAT}.upright found no floor among the volume's {len(run.planes)} planes within "
                         f"{up.get('max_tilt_deg', 35.0)} degrees of up_hint {run.up_hint.tolist()}")
    run.upright = _planes.upright_volume(run.vol, run.floor, None, up.get("up_axis", 2), up.get("up_sign", 1),
                                         up.get("heading"), planes=run.planes)


def find_objects(run, args):
    ob, find_args = args                                       # the run's own volume: resampling loses the floor's samples
    structure, _ = _objects.structure_planes(run.planes, run.floor, ob.get("min_area_m2", 2.0))
    run.objects = run.vol.find_objects(structure, up=run.up_hint if run.floor is None else run.floor,
                                       min_weight=run.min_weight, **find_args)


def write_planes(run, pc):
    run.write("metrics_tsdf_planes.txt", _planes.planes_text(run.planes, run.floor))
    run.report(dict(tsdf_planes_found=len(run.planes), tsdf_floor_found=run.floor is not None),
               f"TSDF planes: {len(run.planes)} found, floor " + (
                   "none" if run.floor is None else
                   f"normal {run.floor['normal'].tolist()!r} offset {run.floor['offset']!r}"))


def write_upright(run, up):
    """Also where the keys under `esdf` learn their frame: `nav_vol` and `nav_c2w`, until here the run's own."""
    run.nav_vol, to_map = run.upright
    if run.c2w_list is not None:
        run.nav_c2w = _planes.moved_poses(to_map, run.c2w_list)
    run.write("map/upright.txt", _planes.transform_text(to_map))
    if up.get("save_volume", False):
        run.nav_vol.save(run.path("mesh/tsdf_upright_volume.npz"))


def nav_boxes(run):
    """The objects' boxes in the frame of `nav_vol`."""
    return run.objects.boxes if run.upright is None else _objects.moved_objects(run.objects, run.upright[1])


def write_objects(run, args):
    boxes = run.objects.boxes
    run.write("map/objects.txt", _objects.objects_text(boxes, None if run.upright is None else nav_boxes(run)))
    on_floor = 0 if run.floor is None else sum(1 for b in boxes if 0 in b["touches"])
    run.report(dict(tsdf_objects_found=len(boxes), tsdf_objects_on_floor=on_floor),
               f"TSDF objects: {len(boxes)} found in {run.objects.n_clusters} clusters, {on_floor} on the floor")


def check_eval_depth(run):
    """tsdf.eval_depth = {enable, every 5, save_images} (absent by default): the run's own volume is raycast at the
    poses of every `every`-th frame of the stream and compared with the sensor depth (tsdf.eval_tsdf_depth) into
    metrics_tsdf_depth.txt, with save_images tsdf_eval/{i:05d}.jpg beside it.  stats: tsdf_depth_l1_cm, tsdf_coverage,
    tsdf_n_frames.  Refuses nothing before the fusion; a missing stream or pose list is refused late, after the mesh,
    planes, upright and objects files are written."""
    return _on(run.opt.get("eval_depth"))


def write_eval_depth(run, ev):
    if run.stream is None or run.c2w_list is None:
        raise ValueError(f"{WHAT}.eval_depth needs the stream and its camera-to-world poses")
    res = _tsdf.eval_tsdf_depth(run.vol, run.stream, run.c2w_list, run.intrinsics(), every=ev.get("every", 5),
                                out_path=run.path("metrics_tsdf_depth.txt"), save_images=ev.get("save_images", False),
                                min_weight=run.min_weight, metric_depth=run.slam.mode == "rgbd")
    run.report({f"tsdf_{k}": res[k] for k in _tsdf.DEPTH_REPORT_ORDER},
               "TSDF depth: " + ", ".join(f"{k} {res[k]!r}" for k in _tsdf.DEPTH_REPORT_ORDER))


def write_mesh(run, _):
    os.makedirs(run.path("mesh"), exist_ok=True)
    run.mesh.export(run.path("mesh/tsdf_mesh.ply"))


def write_volume(run, _):
    """tsdf.save_volume (a bool, absent by default): the run's own volume goes to mesh/tsdf_volume.npz
    (TSDFVolume.save), what tsdf.merge.volume of a later run reads.  No stats, no refusal."""
    run.vol.save(run.path("mesh/tsdf_volume.npz"))


def write_mesh_eval(run, meshing):
    """With meshing.eval_rec and a readable meshing.gt_mesh_path (a .ply) the fused mesh is aligned to that mesh from
    `trans_init` and evaluated into metrics_tsdf_mesh.txt (neus.mesh_eval; n_points_to_eval, mesh_threshold_to_eval).
    No stats, no refusal: without such a file, or with an empty mesh, nothing happens."""
    gt_path = meshing.get("gt_mesh_path") or ""
    if meshing.get("eval_rec") and gt_path.find(".ply") > -1 and os.path.exists(gt_path) and len(run.mesh.faces) > 0:
        from .neus.mesh import load_mesh
        from .neus.mesh_eval import align_mesh, eval_mesh
        gt_mesh = load_mesh(gt_path)
        aligned = align_mesh(run.mesh.copy(), gt_mesh, threshold=0.1, trans_init=run.trans_init)
        eval_mesh(aligned, gt_mesh, N3d=meshing.get("n_points_to_eval", 200000),
                  dist_th=meshing.get("mesh_threshold_to_eval", 0.05), out_path=run.path("metrics_tsdf_mesh.txt"))


def write_esdf(run, ed):
    """tsdf.esdf = {enable, max_distance, save_volume, slice, plan, frontiers, next_view, rooms, floor, scan, mcl} (absent by
    default): the distance field of the volume (TSDFVolume.esdf) and the clearance of the camera centres in it go to
    metrics_tsdf_clearance.txt (tsdf.trajectory_clearance), with save_volume the field to mesh/tsdf_esdf.npz (dist,
    state, lo, voxel), and with slice = {up_axis, height, robot_radius 0, known_fraction 0.5} the map of that slab to
    map/occupancy.pgm and occupancy.yaml (ESDF.save_map).  stats: tsdf_clearance_min_m, tsdf_clearance_inside,
    tsdf_clearance_unknown.  Refuses nothing before the fusion; a missing pose list is refused late, after eval_depth's
    file."""
    if run.c2w_list is None:
        raise ValueError(f"{WHAT}.esdf needs the run's camera-to-world poses")
    field = run.field = run.nav_vol.esdf(ed.get("max_distance"), min_weight=run.min_weight)
    res = _tsdf.trajectory_clearance(field, run.nav_c2w, out_path=run.path("metrics_tsdf_clearance.txt"))
    run.report(dict(tsdf_clearance_min_m=res["clearance_min_m"], tsdf_clearance_inside=res["n_inside"],
                    tsdf_clearance_unknown=res["n_unknown"]),
               "TSDF clearance: " + ", ".join(f"{k} {res[k]!r}" for k in _tsdf.CLEARANCE_REPORT_ORDER))
    if ed.get("save_volume", False):
        np.savez(run.path("mesh/tsdf_esdf.npz"), dist=field.dist.cpu().numpy(), state=field.state.cpu().numpy(),
                 lo=field.lo, voxel=field.voxel)
    sl = ed.get("slice")
    if sl:
        field.save_map(run.path("map"), sl["up_axis"], sl["height"], sl.get("robot_radius", 0.0),
                       sl.get("known_fraction", 0.5))


def check_plan(run):
    """tsdf.esdf.plan = {enable, robot_radius 0, allow_unknown false, snap 0, start "last", goal "first", straighten,
    follow} (absent by default; start and goal are world points or "last" / "first", the run's last and first camera
    centre: by default the way home): the route of ESDF.plan goes to map/path.txt (plan.path_text); with straighten (a
    bool or {enable, window}) its waypoints by straight legs to map/path_straight.txt (plan.straight_path_text); with
    follow = {enable, up_axis, heading, max_ticks, goal_tolerance and follow.Controller's keys; robot_radius and
    allow_unknown default to the plan's} the closed-loop drive of ESDF.follow between the route's two end cells to
    map/follow.txt (follow.follow_text).  stats: tsdf_path_reachable, tsdf_path_length_m; tsdf_path_straight_length_m,
    tsdf_path_waypoints; tsdf_follow_reached, tsdf_follow_ticks, tsdf_follow_min_clearance_m.  Refuses before the fusion
    a bad straighten, then a bad follow; late, after the esdf files, "last" / "first" without a pose."""
    pl = _on(run.esdf.get("plan"))
    if pl is None:
        return None
    return (pl, _plan.straighten_config(pl.get("straighten"), f"{WHAT}.esdf.plan.straighten"),
            _follow.follow_config(pl.get("follow"), f"{WHAT}.esdf.plan.follow"))


def write_plan(run, args):
    pl, window, follow = args
    ends = [run.map_point(pl.get("start", "last")), run.map_point(pl.get("goal", "first"))]      # both moved, then named
    ends = [run.camera_point(end, "plan", ("last", "first")) for end in ends]
    res = run.planned = run.field.plan(ends[0], ends[1], robot_radius=pl.get("robot_radius", 0.0),
                                       allow_unknown=pl.get("allow_unknown", False), snap=pl.get("snap", 0.0),
                                       **({} if window is None else {"straighten": True, "window": window}))
    run.write("map/path.txt", _plan.path_text(res))
    run.report(dict(tsdf_path_reachable=res["reachable"], tsdf_path_length_m=res["length_m"]))
    if window is not None:
        run.write("map/path_straight.txt", _plan.straight_path_text(res))
        run.report(dict(tsdf_path_straight_length_m=res["straight_length_m"],
                        tsdf_path_waypoints=int(res["waypoints"].shape[0])),
                   f"TSDF straightened path: length_m {res['straight_length_m']!r}, min_clearance_m "
                   f"{res['straight_min_clearance_m']!r}, {int(res['waypoints'].shape[0])} waypoints")
    print(f"TSDF path: reachable {res['reachable']!r}, length_m {res['length_m']!r}, "
          f"min_clearance_m {res['min_clearance_m']!r}, {int(res['cells'].shape[0])} points")
    if follow is None:
        return
    drove = _follow.no_drive()
    if res["start_cell"] is not None and res["goal_cell"] is not None:
        # between the cells the route was planned between: camera centres usually sit in cells that do not pass
        field, lo = run.field, torch.tensor(run.field.lo, dtype=torch.float64)
        drive_args = dict(follow[1])
        drive_args.setdefault("robot_radius", pl.get("robot_radius", 0.0))
        drive_args.setdefault("allow_unknown", pl.get("allow_unknown", False))
        drove = field.follow(lo + torch.tensor(res["start_cell"], dtype=torch.float64) * field.voxel,
                             lo + torch.tensor(res["goal_cell"], dtype=torch.float64) * field.voxel,
                             follow[0], **drive_args)
    run.write("map/follow.txt", _follow.follow_text(drove))
    run.report(dict(tsdf_follow_reached=drove["reached"], tsdf_follow_ticks=drove["ticks"],
                    tsdf_follow_min_clearance_m=drove["min_clearance_m"]),
               f"TSDF follow: reached {drove['reached']!r}, ticks {drove['ticks']!r}, length_m {drove['length_m']!r}, "
               f"min_clearance_m {drove['min_clearance_m']!r}, stops {drove['stops']!r}")


def check_frontiers(run):
    """tsdf.esdf.frontiers = {enable, robot_radius 0, min_cells 1, start "last", snap 0, order "nearest"} (absent by
    default; start is a world point or "last"): the frontier clusters of ESDF.frontiers go to map/frontiers.txt
    (frontier.frontiers_text) and, when ESDF.explore finds a goal, its route to map/explore_path.txt (plan.path_text).
    stats: tsdf_frontier_cells, tsdf_frontier_clusters, tsdf_unknown_fraction, tsdf_explore_reachable.  Refuses nothing
    before the fusion; late, after plan's files, a start that is another name and "last" without a pose."""
    return _on(run.esdf.get("frontiers"))


def write_frontiers(run, fr):
    start = run.camera_point(run.map_point(fr.get("start", "last")), "frontiers", ("last",))
    res = run.field.explore(start, robot_radius=fr.get("robot_radius", 0.0), snap=fr.get("snap", 0.0),
                            min_cells=fr.get("min_cells", 1), order=fr.get("order", "nearest"))
    report = _frontier.summary(res["clusters"], res["cluster"])
    run.write("map/frontiers.txt", _frontier.frontiers_text(report))
    if res["reachable"]:
        run.write("map/explore_path.txt", _plan.path_text(res))
    run.report(dict(tsdf_frontier_cells=report["n_frontier"], tsdf_frontier_clusters=report["n_clusters"],
                    tsdf_unknown_fraction=report["unknown_fraction"], tsdf_explore_reachable=res["reachable"]),
               f"TSDF frontiers: {report['n_frontier']} cells in {report['n_clusters']} clusters, {report['n_kept']} "
               f"kept, {report['n_reachable']} reachable, unknown_fraction {report['unknown_fraction']!r}, "
               f"chosen {report['cluster']!r}")


def check_next_view(run):
    """tsdf.esdf.next_view = {enable, camera, up_axis, height, n_yaw 8, robot_radius 0, stride 4, snap 0, start "last",
    lam 0, min_gain_cells 1, min_solid_cells 0, max_unknown 0} (absent by default; start is a world point or "last"):
    the pose of ESDF.next_view goes to map/next_view.txt (view.next_view_text) and, when a view is found, its route to
    map/next_view_path.txt (plan.path_text).  stats: tsdf_next_view_found, tsdf_next_view_gain_m3,
    tsdf_next_view_candidates.  Refuses nothing before the fusion; late, after the frontier files, a start that is
    another name, "last" without a pose, and a missing camera, up_axis or height (a KeyError)."""
    return _on(run.esdf.get("next_view"))


def write_next_view(run, nv):
    start = run.camera_point(run.map_point(nv.get("start", "last")), "next_view", ("last",))
    res = run.field.next_view(start, nv["camera"], nv["up_axis"], nv["height"], n_yaw=nv.get("n_yaw", 8),
                              robot_radius=nv.get("robot_radius", 0.0), stride=nv.get("stride", 4),
                              snap=nv.get("snap", 0.0), max_unknown=nv.get("max_unknown", 0),
                              min_gain_cells=nv.get("min_gain_cells", 1), min_solid_cells=nv.get("min_solid_cells", 0),
                              lam=nv.get("lam", 0.0))
    run.write("map/next_view.txt", _view.next_view_text(res))
    if res["view_cell"] is not None:
        run.write("map/next_view_path.txt", _plan.path_text(res))
    run.report(dict(tsdf_next_view_found=res["view_cell"] is not None, tsdf_next_view_gain_m3=res["gain_m3"],
                    tsdf_next_view_candidates=res["n_candidates"]),
               f"TSDF next view: cell {res['view_cell']!r}, yaw {res['yaw']!r}, gain_m3 {res['gain_m3']!r}, "
               f"{res['n_candidates']} candidates, {res['n_qualified']} qualified")


def check_rooms(run):
    """tsdf.esdf.rooms = {enable, robot_radius 0, core_radius 0.6, min_core_m3, snap 0} (absent by default): the rooms
    and doorways of ESDF.rooms go to map/rooms.txt (rooms.rooms_text): with tsdf.objects on the file lists the room of
    every object (in the map frame when upright), with plan on and its goal reachable the rooms and doorways along
    map/path.txt, and camera_room is the room of the last camera centre, moved by `snap` metres to a cell the robot may
    be at.  stats: tsdf_rooms_found, tsdf_doors_found.  Refuses before the fusion values that are no numbers with
    0 <= robot_radius < core_radius (within esdf.max_distance), min_core_m3 > 0 and snap >= 0, and unknown keys."""
    rm = _on(run.esdf.get("rooms"))
    return None if rm is None else _rooms.config_arguments(rm, run.voxel_size, run.esdf.get("max_distance"))


def write_rooms(run, rm):
    res = run.field.rooms(robot_radius=rm["robot_radius"], core_radius=rm["core_radius"], min_core_m3=rm["min_core_m3"])
    here = None
    if len(run.c2w_list) > 0:
        here = _rooms.room_of_point(res, torch.as_tensor(run.nav_c2w[-1])[:3, 3].double().tolist(), rm["snap"])
    planned = run.planned
    along = res.rooms_along(planned["cells"]) if planned is not None and planned["reachable"] else None
    report = _rooms.summary(res, None if run.objects is None else nav_boxes(run), along, here)
    run.write("map/rooms.txt", _rooms.rooms_text(report))
    run.report(dict(tsdf_rooms_found=report["n_rooms"], tsdf_doors_found=report["n_doors"]),
               f"TSDF rooms: {report['n_rooms']} rooms and {report['n_doors']} doorways over {report['n_open']} open "
               f"cells, {report['n_core']} of them core, camera in room {report['camera_room']!r}")


def check_floor(run):
    """tsdf.esdf.floor = {enable, up_axis, up_sign 1, height, robot_radius, robot_height, step_height, plan false}
    (absent by default; floor.floor_config): the drivable-floor map of ESDF.floor_map goes to map/floor/occupancy.pgm and
    occupancy.yaml (tsdf.save_map) and its areas to map/floor.txt (floor.floor_text); with floor.plan the route of
    plan.plan_on_map on that map between the end cells of map/path.txt, put on the floor by floor.lift, goes to
    map/floor_path.txt (plan.path_text; written unreachable when those cells are missing).  stats:
    tsdf_floor_map_drivable_m2, tsdf_floor_map_unknown_m2; tsdf_floor_path_reachable, tsdf_floor_path_length_m.  Refuses
    before the fusion a bad value, then floor.plan without esdf.plan."""
    if not run.esdf:
        return None
    fm = _floor.floor_config(run.esdf.get("floor"), run.voxel_size)
    if fm is not None and fm["plan"] and _on(run.esdf.get("plan")) is None:
        raise ValueError(f"{WHAT}.esdf.floor.plan replans the route of tsdf.esdf.plan, which is off")
    return fm


def write_floor(run, fm):
    field, planned = run.field, run.planned
    grid = field.floor_map(fm["up_axis"], fm["height"], fm["robot_radius"], fm["robot_height"], fm["step_height"],
                           fm["up_sign"])
    report = _floor.summary(grid)
    _tsdf.save_map(run.path("map/floor"), grid)                # save_map's file names are fixed: a directory of its own
    run.write("map/floor.txt", _floor.floor_text(report))
    run.report(dict(tsdf_floor_map_drivable_m2=report["drivable_m2"], tsdf_floor_map_unknown_m2=report["unknown_m2"]),
               "TSDF floor map: " + ", ".join(f"{k} {report[k]!r}" for k in _floor.FLOOR_REPORT_ORDER))
    if not fm["plan"]:
        return
    route = {"reachable": False, "length_m": math.inf, "points": np.zeros((0, 3))}
    if planned["start_cell"] is not None and planned["goal_cell"] is not None:
        u, v = grid["axes"]                                    # between the cells of the 3-D route, as plan.follow does
        ends = [(field.lo[u] + cell[u] * field.voxel, field.lo[v] + cell[v] * field.voxel)
                for cell in (planned["start_cell"], planned["goal_cell"])]
        res = _plan.plan_on_map(grid, ends[0], ends[1])
        if res["reachable"]:
            route = {"reachable": True, "length_m": res["length_m"], "points": _floor.lift(grid, res["cells"])}
    route["min_clearance_m"] = math.nan                        # the floor map has no clearance field
    run.write("map/floor_path.txt", _plan.path_text(route))
    run.report(dict(tsdf_floor_path_reachable=route["reachable"], tsdf_floor_path_length_m=route["length_m"]),
               f"TSDF floor path: reachable {route['reachable']!r}, length_m {route['length_m']!r}, "
               f"{int(route['points'].shape[0])} points")


def check_scan(run):
    """tsdf.esdf.scan = {up_axis, height, beams 360, fov_deg 360, max_range, every 5, n_yaw 360, window_m 1} (absent by
    default, on whenever present; scan.scan_config): on the occupancy slice at robot radius 0 of those layers a range
    scan is cast at every `every`-th pose whose cell is free (the camera centre on the map's two axes, the yaw of the
    optical axis projected onto them) and found again by scan.localize_on_map within window_m metres over all n_yaw
    yaws, into map/scan_localize.txt (scan.scan_localize_text).  stats: tsdf_scan_poses_tried,
    tsdf_scan_poses_recovered.  Refuses before the fusion an unknown key and a bad value."""
    return _scan.scan_config(run.esdf.get("scan")) if run.esdf else None


def write_scan(run, sc):
    grid = run.field.occupancy_slice(sc["up_axis"], sc["height"], 0.0)
    report = _scan.localize_poses(grid, _scan.planar_poses(run.nav_c2w, grid["axes"]), sc)
    run.write("map/scan_localize.txt", _scan.scan_localize_text(report))
    run.report(dict(tsdf_scan_poses_tried=report["poses_tried"], tsdf_scan_poses_recovered=report["poses_recovered"]),
               "TSDF scan localisation: " + ", ".join(f"{k} {report[k]!r}" for k in _scan.SCAN_SUMMARY_ORDER))


def check_mcl(run):
    """tsdf.esdf.mcl = {up_axis, height, beams 360, fov_deg 360, max_range, every 5, particles 2048, headings 360,
    drift {scale 1, yaw_deg_per_m 0}, seed 0} (absent by default, on whenever present; mcl.mcl_config): on the occupancy
    slice at robot radius 0 of those layers a particle filter (mcl.track_on_map) follows every `every`-th pose of the
    run (scan.planar_poses) from a scan cast at each and the odometry between consecutive ones, stretched and turned by
    `drift`, and relocalises by the exhaustive match when it reports itself lost, into map/mcl.txt (mcl.mcl_text).
    stats: tsdf_mcl_ticks, tsdf_mcl_max_error_m, tsdf_mcl_relocalized.  Refuses before the fusion an unknown key and a
    bad value."""
    return _mcl.mcl_config(run.esdf.get("mcl")) if run.esdf else None


def write_mcl(run, mc):
    grid = run.field.occupancy_slice(mc["up_axis"], mc["height"], 0.0)
    report = _mcl.track_poses(grid, _scan.planar_poses(run.nav_c2w, grid["axes"]), mc)
    run.write("map/mcl.txt", _mcl.mcl_text(report))
    run.report(dict(tsdf_mcl_ticks=report["ticks"], tsdf_mcl_max_error_m=report["max_error_m"],
                    tsdf_mcl_relocalized=report["relocalized"]),
               "TSDF particle filter: " + ", ".join(f"{k} {report[k]!r}" for k in _mcl.MCL_SUMMARY_ORDER))


# ---- the driver -------------------------------------------------------------------------------------------------------
def fuse(run):
    """The fusion: tsdf = {enable, bound (mapping.bound), voxel_size 0.05, source "tracked", truncation, min_weight 1}
    -> `vol` and `mesh` (tsdf.fuse_keyframes)."""
    bound = run.opt.get("bound") or run.slam.cfg["mapping"]["bound"]
    run.min_weight = float(run.opt.get("min_weight", 1.0))
    run.vol, run.mesh = _tsdf.fuse_keyframes(run.slam.video, bound, run.voxel_size, source=run.opt.get("source", "tracked"),
                                             trunc=run.opt.get("truncation"), min_weight=run.min_weight)
    run.nav_vol = run.vol


def fuse_from_config(slam, stream=None, trans_init=None, c2w_list=None, stats=None):
    """`SLAM.terminate`'s TSDF step.  With cfg["tsdf"]["enable"]: check every key of cfg["tsdf"] that is on (the
    `check_*` functions, in this order: of two bad keys the earlier one is reported, and nothing is fused or written),
    fuse the run's keyframes (`fuse`), compute what may still refuse (the merge, the planes, the upright volume, the
    objects: nothing is written yet), then write mesh/tsdf_mesh.ply under `slam.output` and every key's files in the
    order of the list below, each adding its `tsdf_*` values to the dict `stats` and printing a line.  `stream` and
    `c2w_list` are the run's frames and their camera-to-world poses.  Returns the Mesh, or None when the key is absent
    or disabled.  What each key reads, writes and refuses: its `check_*` docstring, and DESIGN.md section 37."""
    opt = slam.cfg.get("tsdf") or {}
    if not opt.get("enable", False):
        return None
    run = Run(slam, opt, stream, trans_init, c2w_list, stats)
    merge, align = check_merge(run), check_align(run)
    upright, planes, objects = check_upright(run), check_planes(run), check_objects(run)
    eval_depth, rooms, plan = check_eval_depth(run), check_rooms(run), check_plan(run)
    frontiers, next_view, floor, scan = check_frontiers(run), check_next_view(run), check_floor(run), check_scan(run)
    mcl = check_mcl(run)
    fuse(run)
    stages = [(join_merge, merge), (find_planes, run.level), (stand_upright, upright),
              (find_objects, objects),                         # what may still refuse; from here on files are written
              (write_mesh, True), (write_planes, planes), (write_upright, upright), (write_objects, objects),
              (write_eval_depth, eval_depth), (write_esdf, run.esdf or None), (write_plan, plan),
              (write_frontiers, frontiers), (write_next_view, next_view), (write_rooms, rooms), (write_floor, floor),
              (write_scan, scan), (write_mcl, mcl), (write_volume, opt.get("save_volume") or None), (write_merge, merge),
              (write_align, align), (write_mesh_eval, slam.cfg.get("meshing") or None)]
    for stage, args in stages:                                 # None: the stage's key is off
        if args is not None:
            stage(run, args)
    return run.mesh
