"""Small deterministic dataset folders in each layout the readers support, shared by tests/golden/gen_golden_datasets.py
(which runs the reference's own classes on them) and the dataset tests (which rebuild them under tmp_path).

Every layout is a dozen frames of smooth images with noise (about 40 x 56; EuRoC's are 752 x 480 greyscale, the size
its rectification maps are made for).  Timestamps are chosen so that association drops frames (TUM: an image without
depth, one without pose; EuRoC: images without an exactly matching pose) and TUM's 32 fps thinning drops every other
one.  CASES names (layout, cfg, args) for each case the fixture records.
"""
import os
import types

import numpy as np
from PIL import Image

N = 12
H, W = 40, 56


def _rng(tag):
    return np.random.default_rng(sum(map(ord, tag)) * 7919)


def _image(g, h, w, c):
    yy, xx = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
    base = [np.sin(3 * xx + g.uniform(0, 6)) * np.cos(2 * yy + g.uniform(0, 6)) for _ in range(c)]
    img = 127.5 + 100 * np.stack(base, -1) + g.normal(0, 12, (h, w, c))
    img = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    return img[:, :, 0] if c == 1 else img


def _depth(g, h, w):
    yy, xx = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
    d = 9000 + 6000 * xx * yy + g.integers(0, 3000, (h, w))
    d[g.random((h, w)) < 0.05] = 0
    return d.astype(np.uint16)


def _save_color(path, img, quality=95):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    im = Image.fromarray(img)
    if path.endswith(".jpg"):
        im.save(path, quality=quality)
    else:
        im.save(path)


def _save_depth(path, d):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(d).save(path)          # uint16 -> a 16-bit greyscale PNG


def _quat(g):
    q = g.normal(size=4)
    q[3] += 3.0                            # near identity, w positive
    return q / np.linalg.norm(q)


def _c2w(g):
    from scipy.spatial.transform import Rotation
    T = np.eye(4)
    T[:3, :3] = Rotation.from_quat(_quat(g)).as_matrix()
    T[:3, 3] = g.normal(size=3)
    return T


def _mat_lines(T, sep=" "):
    return "".join(sep.join(f"{v:.9f}" for v in row) + "\n" for row in T)


def write_replica(root):
    g = _rng("replica")
    for i in range(N):
        _save_color(os.path.join(root, "results", f"frame{i:06d}.jpg"), _image(g, H, W, 3))
        _save_depth(os.path.join(root, "results", f"depth{i:06d}.png"), _depth(g, H, W))
    with open(os.path.join(root, "traj.txt"), "w") as f:
        for _ in range(N):
            f.write(" ".join(f"{v:.9f}" for v in _c2w(g).reshape(-1)) + "\n")


def write_scannet(root):
    """colour 48 x 64 (larger than depth, as ScanNet's), unpadded numeric names (sorting by number matters)"""
    g = _rng("scannet")
    for i in range(N):
        _save_color(os.path.join(root, "color", f"{i}.jpg"), _image(g, 48, 64, 3))
        _save_depth(os.path.join(root, "depth", f"{i}.png"), _depth(g, H, W))
        os.makedirs(os.path.join(root, "pose"), exist_ok=True)
        with open(os.path.join(root, "pose", f"{i}.txt"), "w") as f:
            f.write(_mat_lines(_c2w(g)))


def write_azure(root):
    g = _rng("azure")
    os.makedirs(os.path.join(root, "scene"), exist_ok=True)
    with open(os.path.join(root, "scene", "trajectory.log"), "w") as f:
        for i in range(N):
            _save_color(os.path.join(root, "color", f"{i:05d}.jpg"), _image(g, H, W, 3))
            _save_depth(os.path.join(root, "depth", f"{i:05d}.png"), _depth(g, H, W))
            f.write(f"{i} {i} {i + 1}\n" + _mat_lines(_c2w(g)))


def _tum_lists(root, g, t_img, t_depth, t_pose):
    os.makedirs(root, exist_ok=True)
    with open(os.path.join(root, "rgb.txt"), "w") as f:
        f.write("# color images\n# file: 'test.bag'\n# timestamp filename\n")
        for i, t in enumerate(t_img):
            name = f"rgb/{t:.6f}.png"
            _save_color(os.path.join(root, name), _image(g, H, W, 3))
            f.write(f"{t:.6f} {name}\n")
    with open(os.path.join(root, "depth.txt"), "w") as f:
        f.write("# depth maps\n# file: 'test.bag'\n# timestamp filename\n")
        for t in t_depth:
            name = f"depth/{t:.6f}.png"
            _save_depth(os.path.join(root, name), _depth(g, H, W))
            f.write(f"{t:.6f} {name}\n")
    if t_pose is not None:
        with open(os.path.join(root, "groundtruth.txt"), "w") as f:
            f.write("# ground truth trajectory\n# file: 'test.bag'\n# timestamp tx ty tz qx qy qz qw\n")
            for t in t_pose:
                v = np.concatenate([g.normal(size=3), _quat(g)])
                f.write(f"{t:.4f} " + " ".join(f"{x:.6f}" for x in v) + "\n")


def write_tum(root):
    """images every 20 ms (32 fps thinning keeps every other one), an image with no depth within 80 ms (100.5) and one
    with no pose (100.9)"""
    g = _rng("tum")
    t_img = [100.0 + 0.02 * i for i in range(N)] + [100.5, 100.9]
    t_depth = [100.0 + 0.02 * i + 0.003 for i in range(N)] + [100.901]
    t_pose = [100.0 + 0.01 * k for k in range(31)]
    _tum_lists(root, g, t_img, t_depth, t_pose)


def write_eth3d(root, poses=True):
    """images every 50 ms; with poses, image 4 has none within 80 ms; without, the last image is 52 ms from any
    depth (kept)"""
    g = _rng("eth3d" + str(poses))
    t_img = [10.0 + 0.05 * i for i in range(N)]
    t_depth = [10.0 + 0.05 * i + 0.002 for i in range(N - 1)]
    t_pose = [10.0 + 0.05 * i - 0.001 for i in range(N) if i not in (3, 4, 5)] if poses else None
    _tum_lists(root, g, t_img, t_depth, t_pose)


EUROC_SCENE = "MH_test"


def write_euroc(root):
    """root must end in EUROC_SCENE (the pose list is <scene>/<scene>.txt); greyscale 752 x 480 PNGs for cam0 and cam1,
    nanosecond names; two images have no pose with the same timestamp"""
    g = _rng("euroc")
    os.makedirs(root, exist_ok=True)
    t0 = 1403636579763555584
    stamps = [t0 + 50_000_000 * i for i in range(N)]
    for t in stamps:
        for cam in ("cam0", "cam1"):
            _save_color(os.path.join(root, "mav0", cam, "data", f"{t}.png"), _image(g, 480, 752, 1))
    with open(os.path.join(root, f"{EUROC_SCENE}.txt"), "w") as f:
        f.write("#timestamp tx ty tz qx qy qz qw\n")
        for i, t in enumerate(stamps):
            if i in (3, 8):
                continue
            v = np.concatenate([g.normal(size=3), _quat(g)])
            f.write(f"{t} " + " ".join(f"{x:.9f}" for x in v) + "\n")


def _cfg(dataset, mode, stride, H_, W_, H_out, W_out, H_edge, W_edge, scale, fx=30.0, fy=31.0, cx=27.5, cy=19.5):
    return {"dataset": dataset, "mode": mode, "stride": stride, "data": {"input_folder": None},
            "cam": {"H": H_, "W": W_, "fx": fx, "fy": fy, "cx": cx, "cy": cy, "png_depth_scale": scale,
                    "H_out": H_out, "W_out": W_out, "H_edge": H_edge, "W_edge": W_edge}}


EUROC_CAM = dict(fx=435.2046959714599, fy=435.2046959714599, cx=367.4517211914062, cy=252.2008514404297)

# case -> (folder writer, folder name, cfg, max_frames)
CASES = {
    "replica": (write_replica, "replica", _cfg("replica", "rgbd", 1, H, W, 24, 32, 0, 0, 6553.5), -1),
    "replica_s3": (write_replica, "replica", _cfg("replica", "mono", 3, H, W, 30, 44, 0, 0, 6553.5), -1),
    "scannet": (write_scannet, "scannet", _cfg("scannet", "rgbd", 2, H, W, 16, 24, 4, 4, 1000.0), 9),
    "tum": (write_tum, "tum", _cfg("tumrgbd", "rgbd", 1, H, W, 24, 40, 2, 4, 5000.0), -1),
    "eth3d": (write_eth3d, "eth3d", _cfg("eth3d", "rgbd", 1, H, W, 32, 48, 2, 2, 5000.0), -1),
    "eth3d_nopose": (lambda r: write_eth3d(r, poses=False), "eth3d_nopose",
                     _cfg("eth3d", "rgbd", 2, H, W, 32, 48, 2, 2, 5000.0), -1),
    "euroc": (write_euroc, EUROC_SCENE, _cfg("euroc", "stereo", 1, 480, 752, 24, 32, 2, 2, 0.0, **EUROC_CAM), -1),
    "euroc_mono": (write_euroc, EUROC_SCENE, _cfg("euroc", "mono", 2, 480, 752, 24, 32, 2, 2, 0.0, **EUROC_CAM), -1),
    "azure": (write_azure, "azure", _cfg("azure", "rgbd", 1, H, W, 28, 40, 0, 0, 1000.0), -1),
}


def build(case, parent):
    """Write case's folder under `parent` (once per folder name) -> (cfg, args) pointing at it."""
    writer, name, cfg, max_frames = CASES[case]
    root = os.path.join(parent, name)
    if not os.path.isdir(root):
        writer(root)
    cfg = {**cfg, "data": {"input_folder": root}}
    return cfg, types.SimpleNamespace(input_folder=None, max_frames=max_frames)
