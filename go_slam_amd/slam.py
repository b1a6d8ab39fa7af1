"""The orchestrator: `SLAM(args, cfg)` builds every worker of this package on one set of shared buffers, `run(stream)`
drives them over a sequence and `terminate()` writes the run's outputs (reference src/slam.py).

The reference spawns six processes that spin on shared flags (slam.py:373-390).  Here the same workers run in ONE
process in a fixed order, which is deterministic under a seed; see `SLAM.run` for what each step corresponds to.
"""
import os
from collections import OrderedDict
from time import gmtime, strftime

import numpy as np
import torch
import torch.nn as nn

from . import traj_eval
from .backend import Backend
from .depth_video import DepthVideo
from .droid_net import DroidNet
from .frontend import Frontend
from .motion_filter import MotionFilter
from .multiview_filter import MultiviewFilter
from .neus import InstantNeuS, Renderer
from .neus.mapping import Mapper
from .neus.mesher import Mesher
from .trajectory_filler import PoseTrajectoryFiller

FLAGS = ("num_running_thread", "all_trigered", "tracking_finished", "mapping_finished", "meshing_finished",
         "optimizing_finished", "visualizing_finished", "hang_on", "reload_map")
MESH_EVERY = 50        # with make_video, timestamps at which a mesh is extracted (slam.py:220-221)


class Tracker(nn.Module):
    """Motion filter, then the frontend's local bundle adjustment, for one incoming frame (slam.py:26-51)."""

    def __init__(self, cfg, args, slam):
        super().__init__()
        self.args, self.cfg = args, cfg
        self.device = args.device
        self.net, self.video, self.verbose = slam.net, slam.video, slam.verbose
        self.frontend_window = cfg["tracking"]["frontend"]["window"]
        self.motion_filter = MotionFilter(self.net, self.video, thresh=cfg["tracking"]["motion_filter"]["thresh"],
                                          device=self.device)
        self.frontend = Frontend(self.net, self.video, self.args, self.cfg)

    def forward(self, timestamp, image, depth, intrinsic, gt_pose=None):
        with torch.no_grad():
            self.motion_filter.track(timestamp, image, depth, intrinsic, gt_pose=gt_pose)
            self.frontend()


class BundleAdjustment(nn.Module):
    """Full bundle adjustment over every keyframe, once there are more of them than the frontend's window
    (slam.py:54-88)."""

    def __init__(self, cfg, args, slam):
        super().__init__()
        self.args, self.cfg = args, cfg
        self.device = args.device
        self.net, self.video, self.verbose = slam.net, slam.video, slam.verbose
        self.frontend_window = cfg["tracking"]["frontend"]["window"]
        self.last_t = -1
        self.ba_counter = -1
        self.backend = Backend(self.net, self.video, self.args, self.cfg)

    def info(self, msg):
        print(msg)

    def forward(self):
        cur_t = self.video.counter.value
        if cur_t > self.frontend_window:
            self.backend.dense_ba(t_start=0, t_end=cur_t, steps=6, motion_only=False)
            if self.verbose:
                self.info(f'{strftime("%Y-%m-%d %H:%M:%S", gmtime())} - Full BA : [0, {cur_t}]; '
                          f"Current Keyframe is {cur_t}, last is {self.last_t}.")
            self.last_t = cur_t


def _valid_pose(pose):
    total = float(np.asarray(pose, dtype=np.float64).sum())
    return not (np.isnan(total) or np.isinf(total))


class SLAM:
    def __init__(self, args, cfg, full_ba_every=10):
        """`full_ba_every`: the in-process schedule calls the full bundle adjustment after every this many new
        keyframes.  It stands in for the reference's optimiser process, which calls it as often as it gets round to
        (slam.py:229-235); the default of 10 is a schedule choice, not a measured number."""
        self.args, self.cfg = args, cfg
        self.device = args.device
        self.verbose = cfg["verbose"]
        self.mode = cfg["mode"]
        self.only_tracking = cfg["only_tracking"]
        self.make_video = args.make_video
        self.full_ba_every = int(full_ba_every)
        self.output = cfg["data"]["output"] if args.output is None else args.output
        os.makedirs(self.output, exist_ok=True)
        os.makedirs(f"{self.output}/logs/", exist_ok=True)

        self.update_cam(cfg)
        self.load_bound(cfg)

        map_dev = cfg["mapping"]["device"]
        self.mapping_net = InstantNeuS(cfg["mapping"]["model"], bound=cfg["mapping"]["bound"], device=map_dev).to(map_dev)
        self.net = DroidNet()
        self.load_pretrained(cfg["tracking"]["pretrained"])
        self.net.to(self.device).eval()

        self.renderer = Renderer(cfg, args, self)
        for name in FLAGS:
            setattr(self, name, torch.zeros(1).int())
        self.post_processing_iters = cfg["mapping"]["post_processing_iters"]

        self.video = DepthVideo(cfg, args)
        self.tracker = Tracker(cfg, args, self)
        self.ba = BundleAdjustment(cfg, args, self)
        self.multiview_filter = MultiviewFilter(cfg, args, self)
        self.traj_filler = PoseTrajectoryFiller(net=self.net, video=self.video, device=self.device)
        self.mapper = Mapper(cfg, args, self)
        self.mesher = Mesher(cfg, args, self)
        from .tsdf_live import live_from_config
        self.live = live_from_config(self)          # None unless cfg["tsdf"]["live"]["enable"]
        self.live_mesh_every = int(((cfg.get("tsdf") or {}).get("live") or {}).get("mesh_every", 0))

    def update_cam(self, cfg):
        """Intrinsics after the preprocessing of the frames: resize to (H_out + 2 H_edge, W_out + 2 W_edge), then crop
        the edges."""
        cam = cfg["cam"]
        h_edge, w_edge = cam["H_edge"], cam["W_edge"]
        H_out, W_out = cam["H_out"], cam["W_out"]
        self.fx = cam["fx"] * (W_out + w_edge * 2) / cam["W"]
        self.fy = cam["fy"] * (H_out + h_edge * 2) / cam["H"]
        self.cx = cam["cx"] * (W_out + w_edge * 2) / cam["W"]
        self.cy = cam["cy"] * (H_out + h_edge * 2) / cam["H"]
        self.H, self.W = H_out, W_out
        self.cx = self.cx - w_edge
        self.cy = self.cy - h_edge

    def load_bound(self, cfg):
        self.bound = torch.from_numpy(np.array(cfg["mapping"]["bound"])).float()

    def load_pretrained(self, pretrained):
        """DROID-SLAM's checkpoint into `self.net`: `module.` prefixes stripped, the weight and delta heads cut to their
        first two output rows.  Without a checkpoint (None or '') the seeded random DroidNet stays."""
        if not pretrained:
            print("INFO: tracking.pretrained is not set, keeping the randomly initialised DroidNet!")
            return
        print(f"INFO: load pretrained checkpoint from {pretrained}!")
        state = OrderedDict((k.replace("module.", ""), v) for k, v in torch.load(pretrained).items())
        for key in ("update.weight.2.weight", "update.weight.2.bias", "update.delta.2.weight", "update.delta.2.bias"):
            state[key] = state[key][:2]
        self.net.load_state_dict(state)

    def run(self, stream):
        """One pass over `stream` in one process.  Against the reference's processes (slam.py:210-287):

          * per frame, `tracker(...)` with the depth dropped unless mode == 'rgbd' -- the loop of `tracking` (:215-218);
          * after a frame that added a keyframe, `multiview_filter()` then `mapper()` -- one round each of the loops of
            `multiview_filtering` (:246-249) and `mapping` (:256-259), which there spin beside the tracker;
          * after every `full_ba_every` new keyframes, `ba()` -- the loop of `optimizing` (:232-235);
          * with cfg["tsdf"]["live"]["enable"], `live.update()` after a frame that added a keyframe and after every
            `ba()` -- no counterpart: the running TSDF volume follows the poses (tsdf_live.LiveFusion; also under
            only_tracking), and with its `mesh_every` > 0 mesh/live/{timestamp:05d}.ply at those timestamps;
          * with make_video, `mesher()` at every 50th timestamp -- `hang_on` and the meshing worker (:220-224, :271-275);
          * after the stream: a last `ba()` (:237-238), one `multiview_filter()`, `post_processing_iters` times
            `mapper(the_end=True)` (:261-264), then the finished flags (:226, :239, :265, :277, :286).

        Nothing but the tracker and the bundle adjustment runs under only_tracking (run's `dont_run`, :374-383)."""
        self.num_running_thread[0] += 1
        self.all_trigered += 1
        since_ba = 0
        live = getattr(self, "live", None)          # (a SLAM assembled without __init__ has none)
        for timestamp, image, depth, intrinsic, gt_pose in stream:
            if self.mode != "rgbd":
                depth = None
            before = self.video.counter.value
            self.tracker(timestamp, image, depth, intrinsic, gt_pose)
            if self.video.counter.value > before:
                since_ba += 1
                if not self.only_tracking:
                    self.multiview_filter()
                    self.mapper()
                if live is not None:
                    live.update()
                if since_ba >= self.full_ba_every:
                    self.ba()
                    since_ba = 0
                    if live is not None:
                        live.update()
            if live is not None and self.live_mesh_every > 0 and timestamp % self.live_mesh_every == 0 and timestamp > 0:
                from .tsdf_live import save_live_mesh
                save_live_mesh(self, f"{self.output}/mesh/live/{int(timestamp):05d}.ply")
            if self.make_video and not self.only_tracking and timestamp % MESH_EVERY == 0 and timestamp > 0:
                self.mesher()
        self.tracking_finished += 1
        self.ba()
        if live is not None:
            live.update()
        self.optimizing_finished += 1
        if not self.only_tracking:
            self.multiview_filter()
            for _ in range(self.post_processing_iters):
                self.mapper(the_end=True)
        self.mapping_finished += 1
        self.meshing_finished += 1
        self.visualizing_finished += 1

    def terminate(self, rank=-1, stream=None):
        """Fill in the poses of the non-keyframes, evaluate the trajectory and write the run's files (slam.py:289-370):
        checkpoints/go.ckpt, checkpoints/est_poses.npy, then submission.txt without ground truth or metrics_traj.txt with
        it, and the final mesh.  With cfg["tsdf"]["enable"] also mesh/tsdf_mesh.ply, the keyframe depth fused into a TSDF
        (this one also under only_tracking), and what the further keys of cfg["tsdf"] ask for, their values under `tsdf_*`
        keys of the returned statistics (tsdf_run.fuse_from_config).  With cfg["tsdf"]["live"]["enable"] the
        running volume is brought to the final poses (LiveFusion.finish) and meshed into mesh/tsdf_live_mesh.ply, and
        `tsdf_live_refused` (keyframes re-fused over the run) and `tsdf_live_keyframes` join the statistics.  With
        cfg["render_eval"]["enable"] (keys enable, every, save_images) and a map, also metrics_render.txt: PSNR, SSIM and depth L1 of the map's renderings against the input
        frames (neus/render_eval.py), their means under `render_*` keys of the returned statistics.  Returns the
        statistics (an empty dict without ground truth and without that step)."""
        os.makedirs(f"{self.output}/checkpoints/", exist_ok=True)
        torch.save({"mapping_net": self.mapping_net.state_dict(), "tracking_net": self.net.state_dict(),
                    "keyframe_timestamps": self.video.timestamp}, f"{self.output}/checkpoints/go.ckpt")
        print("#" * 20 + f" Results for {stream.input_folder} ...")

        w2c = self.traj_filler(stream).data
        tq, c2w = traj_eval.world_poses(w2c, self.video.pose_compensate[0])
        estimate_c2w_list = c2w.float().cpu()          # what the file holds is what gets evaluated and meshed
        np.save(f"{self.output}/checkpoints/est_poses.npy", estimate_c2w_list.numpy())

        stats, trans_init, gt_c2w_list = {}, None, None
        if stream.poses is None:
            if stream.image_timestamps is not None:
                path = f"{self.output}/submission.txt"
                with open(path, "w") as fh:        # timestamp tx ty tz qx qy qz qw
                    for stamp, pose in zip(stream.image_timestamps, tq.float().cpu().tolist()):
                        fh.write(f"{stamp:.9f}" + "".join(f" {v:.14f}" for v in pose) + "\n")
                print(f"Poses are saved to {path}!")
            print("Terminate: no GT poses found!")
        else:
            gt = np.stack([np.asarray(p, dtype=np.float64) for p in stream.poses], axis=0)
            valid = np.array([_valid_pose(p) for p in gt])
            for i in np.nonzero(~valid)[0]:
                print(f"Nan or Inf found in gt poses, skipping {i}th pose!")
            gt_c2w_list = torch.from_numpy(gt[valid])
            dev = c2w.device
            result = traj_eval.ape(estimate_c2w_list[:, :3, 3].to(dev, torch.float64),
                                   torch.from_numpy(np.ascontiguousarray(gt[:, :3, 3])).to(dev),
                                   torch.from_numpy(valid).to(dev))
            with open(f"{self.output}/metrics_traj.txt", "a") as fh:
                fh.write(traj_eval.metrics_text(result))
            trans_init = result["alignment_transformation_sim3"]
            stats = {k: v for k, v in result.items() if k != "errors"}
            print(traj_eval.metrics_text(result))

        if self.meshing_finished > 0 and not self.only_tracking:
            self.mesher(the_end=True, estimate_c2w_list=estimate_c2w_list, gt_c2w_list=gt_c2w_list,
                        trans_init=trans_init)
        render_cfg = self.cfg.get("render_eval") or {}
        if render_cfg.get("enable", False) and not self.only_tracking:     # metrics_render.txt
            from .neus.render_eval import REPORT_ORDER, eval_rendering
            res = eval_rendering(self, stream, estimate_c2w_list, every=render_cfg.get("every", 5),
                                 out_path=f"{self.output}/metrics_render.txt",
                                 save_images=render_cfg.get("save_images", False))
            stats.update({f"render_{k}": res[k] for k in REPORT_ORDER})
            print("Rendering: " + ", ".join(f"{k} {res[k]!r}" for k in REPORT_ORDER))
        if (self.cfg.get("tsdf") or {}).get("enable", False):     # mesh/tsdf_mesh.ply, also under only_tracking
            from .tsdf import fuse_from_config
            fuse_from_config(self, stream=stream, trans_init=trans_init, c2w_list=estimate_c2w_list, stats=stats)
        if getattr(self, "live", None) is not None:               # mesh/tsdf_live_mesh.ply, also under only_tracking
            from .tsdf_live import save_live_mesh
            self.live.finish()
            save_live_mesh(self, f"{self.output}/mesh/tsdf_live_mesh.ply")
            stats.update(tsdf_live_refused=self.live.total["refused"], tsdf_live_keyframes=len(self.live))
        print("Terminate: Done!")
        return stats
