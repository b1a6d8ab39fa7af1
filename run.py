"""Run GO-SLAM on one sequence: python run.py <config.yaml> [--input_folder DIR] [--output DIR] ...

Writes cfg.yaml, checkpoints/go.ckpt, checkpoints/est_poses.npy, metrics_traj.txt (or submission.txt without ground
truth poses) and mesh/ into the output folder.  Arguments are the reference's run.py's, plus --default_config.
"""
import argparse
import os
import random

import numpy as np
import torch

from go_slam_amd import config
from go_slam_amd.datasets import get_dataset
from go_slam_amd.slam import SLAM


def setup_seed(seed):
    torch.manual_seed(seed)
    torch.cuda.manual_seed_all(seed)
    np.random.seed(seed)
    random.seed(seed)
    torch.backends.cudnn.deterministic = True


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("config", type=str, help="Path to config file.")
    parser.add_argument("--device", type=str, default="cuda:0")
    parser.add_argument("--max_frames", type=int, default=-1, help="Only [0, max_frames] Frames will be run")
    parser.add_argument("--only_tracking", action="store_true", help="Only tracking is triggered")
    parser.add_argument("--make_video", action="store_true", help="extract a mesh every 50 frames for a video")
    parser.add_argument("--input_folder", type=str, help="input folder, overrides the one in the config file")
    parser.add_argument("--output", type=str, help="output folder, overrides the one in the config file")
    parser.add_argument("--image_size", nargs="+", default=None, help="image height and width, overrides the config file")
    parser.add_argument("--calibration_txt", type=str, default=None,
                        help="file with fx, fy, cx, cy, overrides the config file")
    parser.add_argument("--mode", type=str, help="slam mode: mono, rgbd or stereo")
    parser.add_argument("--default_config", type=str, default="./configs/go_slam.yaml",
                        help="defaults under the config file's inherit_from chain; skipped when the file does not exist")
    return parser.parse_args(argv)


def main(argv=None):
    setup_seed(43)
    args = parse_args(argv)
    default = args.default_config
    if default is not None and not os.path.exists(default):
        print(f"INFO: default config {default} not found, loading {args.config} without defaults")
        default = None
    cfg = config.load_config(args.config, default)

    if args.mode is not None:
        cfg["mode"] = args.mode
    if args.only_tracking:
        cfg["only_tracking"] = True
    if args.image_size is not None:
        cfg["cam"]["H"], cfg["cam"]["W"] = (int(v) for v in args.image_size)
    if args.calibration_txt is not None:
        cfg["cam"]["fx"], cfg["cam"]["fy"], cfg["cam"]["cx"], cfg["cam"]["cy"] = np.loadtxt(args.calibration_txt).tolist()
    assert cfg["mode"] in ["rgbd", "mono", "stereo"], cfg["mode"]
    print(f"\n\n** Running {cfg['data']['input_folder']} in {cfg['mode']} mode!!! **\n\n")
    print(args)

    output_dir = cfg["data"]["output"] if args.output is None else args.output
    os.makedirs(output_dir, exist_ok=True)
    config.save_config(cfg, f"{output_dir}/cfg.yaml")

    dataset = get_dataset(cfg, args, device=args.device)
    slam = SLAM(args, cfg)
    slam.run(dataset)
    stats = slam.terminate(rank=-1, stream=dataset)
    print("Done!")
    return stats


if __name__ == "__main__":
    main()
