"""Dataset readers (src/datasets.py): a dataset folder -> (index, color [b,3,H,W] in [0,1], depth [H,W] in metres,
intrinsic [4], c2w [4,4]) per frame, the tuples that SLAM.tracking and PoseTrajectoryFiller consume.

The bookkeeping -- globbing and sorting, stride and max_frames, timestamp association, TUM's frame-rate thinning, the
first-pose normalisation, ETH3D's image_timestamps and the intrinsics -- is the reference's, operation for operation.
The pixels are decoded on the host with PIL and everything after decoding runs on the GPU (csrc/frame_prep.hip): the
rectification or undistortion remap, cv2.resize INTER_LINEAR, RGB in [0, 1], the edge crop, depth / png_depth_scale
and the nearest resize.  Raw uint8 / uint16 pixels are uploaded, a quarter of the float32 bytes.

Output placement: MotionFilter.track normalises its input in place on the device copy, so a host image is stored in
the video unnormalised and a device image normalised (the reference's behaviour).  The default `output="host"` therefore
hands out host float32 tensors as the reference does; `output="device"` is for consumers that do not alias.  Every item
is freshly allocated.

Iterating a dataset prefetches: a small pool of decoder threads (PIL releases the GIL while it decodes) runs ahead, and
batches of frames are uploaded from pinned memory and preprocessed on a side stream, one colour and one depth launch
per batch; an event guards the consumer.  DESIGN.md section 17.
"""
import collections
import glob
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
from PIL import Image

from . import _lib

DECODE_THREADS = 4          # decoder pool; deliberately independent of the machine's CPU count
BATCH = 4                   # frames per upload / launch while iterating


def get_dataset(cfg, args, device='cuda:0', **options):
    return dataset_dict[cfg['dataset']](cfg, args, device=device, **options)


# ---------------------------------------------------------------------------------------------------- decoding ----

def read_color(path):
    """uint8 [h, w, 3] RGB or [h, w] grey: what cv2.imread(path) gives, channels reversed (a grey image is what
    cv2.imread repeats into three channels).  PNG is lossless, so the pixels are cv2's; a JPEG decoder may differ from
    cv2's by a level."""
    with Image.open(path) as im:
        if im.mode in ("I;16", "I;16B", "I;16L"):
            return (np.asarray(im).astype(np.uint16) >> 8).astype(np.uint8)      # cv2.IMREAD_COLOR of 16-bit grey
        if im.mode == "L":
            return np.asarray(im)
        if im.mode == "LA":
            return np.asarray(im.convert("L"))
        return np.asarray(im if im.mode == "RGB" else im.convert("RGB"))


def read_depth(path):
    """uint16 [h, w]: cv2.imread(path, IMREAD_UNCHANGED) of a depth PNG."""
    if '.png' not in path:
        if '.exr' in path:
            raise NotImplementedError(f"{path}: EXR depth (CoFusion) is not supported: no EXR reader is available")
        raise TypeError(path)
    with Image.open(path) as im:
        a = np.asarray(im)
    if a.ndim != 2:
        raise ValueError(f"{path}: a depth PNG must have one channel, got shape {a.shape}")
    return a.astype(np.uint16)


# ---------------------------------------------------------------------------------- rectification / undistortion ----

def init_undistort_rectify_map(K, D, R, P, size):
    """cv2.initUndistortRectifyMap(K, D, R, P, (w, h), CV_32F) -> (map_x, map_y) float32 [h, w], in float64 as
    OpenCV's scalar loop computes it (the running sums along a row included).  D = k1 k2 p1 p2 [k3]."""
    w, h = size
    K = np.asarray(K, dtype=np.float64)
    R = np.asarray(R, dtype=np.float64)
    d = np.zeros(5)
    dd = np.asarray(D, dtype=np.float64).reshape(-1)
    d[:min(dd.size, 5)] = dd[:5]
    k1, k2, p1, p2, k3 = d
    ir = np.linalg.inv(np.asarray(P, dtype=np.float64)[:3, :3] @ R).reshape(-1)
    fx, fy, u0, v0 = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    rows = np.arange(h, dtype=np.float64)
    xs, ys, ws = rows * ir[1] + ir[2], rows * ir[4] + ir[5], rows * ir[7] + ir[8]
    map_x = np.empty((h, w), dtype=np.float32)
    map_y = np.empty((h, w), dtype=np.float32)
    for j in range(w):
        inv = 1.0 / ws
        x, y = xs * inv, ys * inv
        x2, y2 = x * x, y * y
        r2 = x2 + y2
        xy2 = 2 * x * y
        kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((0.0 * r2 + 0.0) * r2 + 0.0) * r2)
        map_x[:, j] = fx * (x * kr + p1 * xy2 + p2 * (r2 + 2 * x2) + 0.0 * r2 + 0.0 * r2 * r2) + u0
        map_y[:, j] = fy * (y * kr + p1 * (r2 + 2 * y2) + p2 * xy2 + 0.0 * r2 + 0.0 * r2 * r2) + v0
        xs, ys, ws = xs + ir[0], ys + ir[3], ws + ir[6]
    return map_x, map_y


# EuRoC's stereo rectification (left, right): K, D, R, P -- the calibration the reference hard-codes
EUROC_SIZE = (752, 480)
EUROC_RECT = (
    (np.array([458.654, 0.0, 367.215, 0.0, 457.296, 248.375, 0.0, 0.0, 1.0]).reshape(3, 3),
     np.array([-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05, 0.0]),
     np.array([0.999966347530033, -0.001422739138722922, 0.008079580483432283,
               0.001365741834644127, 0.9999741760894847, 0.007055629199258132,
               -0.008089410156878961, -0.007044357138835809, 0.9999424675829176]).reshape(3, 3),
     np.array([435.2046959714599, 0, 367.4517211914062, 0, 0, 435.2046959714599, 252.2008514404297, 0,
               0, 0, 1, 0]).reshape(3, 4)),
    (np.array([457.587, 0.0, 379.999, 0.0, 456.134, 255.238, 0.0, 0.0, 1]).reshape(3, 3),
     np.array([-0.28368365, 0.07451284, -0.00010473, -3.555907e-05, 0.0]),
     np.array([0.9999633526194376, -0.003625811871560086, 0.007755443660172947,
               0.003680398547259526, 0.9999684752771629, -0.007035845251224894,
               -0.007729688520722713, 0.007064130529506649, 0.999945173484644]).reshape(3, 3),
     np.array([435.2046959714599, 0, 367.4517211914062, -47.90639384423901, 0, 435.2046959714599, 252.2008514404297, 0,
               0, 0, 1, 0]).reshape(3, 4)),
)


def euroc_maps():
    """[(map_x, map_y) of the left view, of the right view]."""
    return [init_undistort_rectify_map(K, D, R, P[:3, :3], EUROC_SIZE) for K, D, R, P in EUROC_RECT]


# ------------------------------------------------------------------------------------------------- bookkeeping ----

def parse_list(filepath, skiprows=0):
    """A space-separated list file as strings ('#' lines are comments)."""
    return np.loadtxt(filepath, delimiter=' ', dtype=np.str_, skiprows=skiprows)


def pose_matrix_from_quaternion(pvec):
    """[tx ty tz qx qy qz qw] -> 4x4 float64 c2w."""
    from scipy.spatial.transform import Rotation
    pose = np.eye(4)
    pose[:3, :3] = Rotation.from_quat(pvec[3:]).as_matrix()
    pose[:3, 3] = pvec[:3]
    return pose


def associate(tstamp_image, tstamp_depth, tstamp_pose, max_dt=0.08, require_depth=True):
    """Nearest depth and pose per image: (i, j, k) when both are within max_dt; with no poses (i, j) -- kept whatever
    the distance unless `require_depth`; with no depth (EuRoC) (i, k) when the pose is within max_dt."""
    out = []
    for i, t in enumerate(tstamp_image):
        if tstamp_pose is None:
            j = np.argmin(np.abs(tstamp_depth - t))
            if not require_depth or np.abs(tstamp_depth[j] - t) < max_dt:
                out.append((i, j))
            continue
        k = np.argmin(np.abs(tstamp_pose - t))
        if tstamp_depth is None:
            if np.abs(tstamp_pose[k] - t) < max_dt:
                out.append((i, k))
            continue
        j = np.argmin(np.abs(tstamp_depth - t))
        if np.abs(tstamp_depth[j] - t) < max_dt and np.abs(tstamp_pose[k] - t) < max_dt:
            out.append((i, j, k))
    return out


def relative_poses(pose_vecs):
    """c2w of every pose vector relative to the first: I, then inv(first) @ c2w."""
    poses, inv_first = [], None
    for v in pose_vecs:
        c2w = pose_matrix_from_quaternion(v)
        if inv_first is None:
            inv_first = np.linalg.inv(c2w)
            c2w = np.eye(4)
        else:
            c2w = inv_first @ c2w
        poses.append(c2w)
    return poses


def _find_pose_list(datapath):
    for name in ('groundtruth.txt', 'pose.txt'):
        if os.path.isfile(os.path.join(datapath, name)):
            return os.path.join(datapath, name)
    return None


def _numeric_sorted(paths):
    return sorted(paths, key=lambda p: int(os.path.basename(p)[:-4]))


class BaseDataset(torch.utils.data.Dataset):
    """cfg / args as the reference reads them.  Options: output = "host" (default, the reference's placement) or
    "device"; decode_threads (default DECODE_THREADS); batch = frames per launch while iterating (default BATCH)."""

    def __init__(self, cfg, args, device='cuda:0', output="host", decode_threads=DECODE_THREADS, batch=BATCH):
        super().__init__()
        if output not in ("host", "device"):
            raise ValueError(f"output must be 'host' or 'device', got {output!r}")
        self.name = cfg['dataset']
        self.stereo = cfg['mode'] == 'stereo'
        self.device = device
        self.output = output
        self.decode_threads = int(decode_threads)
        self.batch = int(batch)
        cam = cfg['cam']
        self.png_depth_scale = cam['png_depth_scale']
        self.n_img = -1
        self.depth_paths = None
        self.color_paths = None
        self.poses = None
        self.image_timestamps = None
        self.H, self.W = cam['H'], cam['W']
        self.fx, self.fy, self.cx, self.cy = cam['fx'], cam['fy'], cam['cx'], cam['cy']
        self.H_out, self.W_out = cam['H_out'], cam['W_out']
        self.H_edge, self.W_edge = cam['H_edge'], cam['W_edge']
        self.distortion = np.array(cam['distortion']) if 'distortion' in cam else None
        self.input_folder = cfg['data']['input_folder'] if args.input_folder is None else args.input_folder
        self.bytes_h2d = 0
        self.bytes_d2h = 0
        self._dev_state = None

    def __len__(self):
        return self.n_img

    # --- what the tests can check without a GPU
    def view_paths(self, index):
        """The colour file(s) of an item: [left] or [left, right]."""
        return [self.color_paths[index]]

    def intrinsic(self):
        """fx fy cx cy of the cropped output, the reference's float32 operations in its order."""
        H_full, W_full = self.H_out + 2 * self.H_edge, self.W_out + 2 * self.W_edge
        intr = torch.as_tensor([self.fx, self.fy, self.cx, self.cy]).float()
        for i, ratio in ((0, W_full / self.W), (1, H_full / self.H), (2, W_full / self.W), (3, H_full / self.H)):
            intr[i] *= ratio
        if self.W_edge > 0:
            intr[2] -= self.W_edge
        if self.H_edge > 0:
            intr[3] -= self.H_edge
        return intr

    def frame_info(self, index):
        """An item's bookkeeping without decoding: colour paths, depth path, pose (float32 [4,4] or None), timestamp
        (ETH3D's image_timestamps, else None) and intrinsic."""
        color = self.view_paths(index)
        return dict(index=index, color_paths=color,
                    depth_path=None if self.depth_paths is None else self.depth_paths[index],
                    pose=None if self.poses is None else torch.from_numpy(self.poses[index]).float(),
                    timestamp=None if self.image_timestamps is None else self.image_timestamps[index],
                    intrinsic=self.intrinsic())

    # --- pixels
    def view_maps(self, view, h, w):
        """(map_x, map_y) of colour view `view` at decoded size h x w, or None: cv2.undistort's map when
        cfg['cam']['distortion'] is set."""
        if self.distortion is None:
            return None
        K = np.array([[self.fx, 0, self.cx], [0, self.fy, self.cy], [0, 0, 1]], dtype=np.float64)
        return init_undistort_rectify_map(K, self.distortion, np.eye(3), K, (w, h))

    def decode(self, index):
        """Host side of one item: ([colour uint8 arrays], depth uint16 array or None)."""
        colors = [read_color(p) for p in self.view_paths(index)]
        depth = None if self.depth_paths is None else read_depth(self.depth_paths[index])
        return colors, depth

    def __getitem__(self, index):
        if not -len(self) <= index < len(self):
            raise IndexError(index)
        index = index % len(self)
        return self.load_batch([index])[0]

    def load_batch(self, indices):
        """The items of `indices`, decoded here and preprocessed in one colour and one depth launch."""
        frames = [(i, self.decode(i)) for i in indices]
        return [item for item, _ in self._prep(frames)] if self.output == "device" else \
            [self._finish(item, ev) for item, ev in self._prep(frames)]

    def __iter__(self):
        return _Prefetcher(self)

    def __getstate__(self):
        state = self.__dict__.copy()
        state['_dev_state'] = None
        return state

    # --- device side
    def _device(self):
        dev = torch.device(self.device)
        if dev.type != 'cuda':
            raise RuntimeError(f"{type(self).__name__}: frame preprocessing runs on the GPU (csrc/frame_prep.hip); "
                               f"device {self.device!r} has no pixels path")
        if self._dev_state is None:
            self._dev_state = dict(stream=torch.cuda.Stream(dev), maps={})
        return dev

    def _maps_on(self, dev, view, h, w):
        key = (view, h, w)
        maps = self._dev_state['maps']
        if key not in maps:
            m = self.view_maps(view, h, w)
            maps[key] = None if m is None else tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in m)
        return maps[key]

    def _prep(self, frames):
        """frames: [(index, (colors, depth))] -> [(item, event)], the work enqueued on the side stream."""
        dev = self._device()
        side = self._dev_state['stream']
        H, W = self.H_out, self.W_out
        views, depths = [], []
        # one pinned staging buffer and one device buffer for all raw pixels of the batch, each array 256-byte aligned
        arrays = []
        for _, (colors, depth) in frames:
            arrays += colors
            if depth is not None:
                arrays.append(depth)
        offs, total = [], 0
        for a in arrays:
            offs.append(total)
            total += (a.nbytes + 255) // 256 * 256
        staging = torch.empty(max(total, 256), dtype=torch.uint8, pin_memory=True)
        host = staging.numpy()
        for a, o in zip(arrays, offs):
            host[o:o + a.nbytes] = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
        self.bytes_h2d += total
        items = []
        with torch.cuda.device(dev), torch.cuda.stream(side):
            raw = torch.empty(staging.numel(), dtype=torch.uint8, device=dev)
            raw.copy_(staging, non_blocking=True)
            base = raw.data_ptr()
            a_i = 0
            tmps = []
            for index, (colors, depth) in frames:
                color = torch.empty(len(colors), 3, H, W, dtype=torch.float32, device=dev)
                for v, img in enumerate(colors):
                    h, w = img.shape[:2]
                    c = 1 if img.ndim == 2 else img.shape[2]
                    cv = _lib.ColorView(src=base + offs[a_i], dst=color[v].data_ptr(), h=h, w=w, c=c)
                    maps = self._maps_on(dev, v, h, w)
                    if maps is not None:
                        mh, mw = maps[0].shape
                        tmp = torch.empty((mh * mw * c + 3) // 4 * 4, dtype=torch.uint8, device=dev)
                        tmps.append(tmp)
                        cv.map_x, cv.map_y, cv.tmp = maps[0].data_ptr(), maps[1].data_ptr(), tmp.data_ptr()
                        cv.mh, cv.mw = mh, mw
                    views.append(cv)
                    a_i += 1
                d_out = None
                if depth is not None:
                    d_out = torch.empty(H, W, dtype=torch.float32, device=dev)
                    depths.append(_lib.DepthView(src=base + offs[a_i], dst=d_out.data_ptr(), h=depth.shape[0],
                                                 w=depth.shape[1]))
                    a_i += 1
                items.append([index, color, d_out])
            L = _lib.lib()
            st = _lib.stream_ptr(dev)
            cvs = (_lib.ColorView * max(len(views), 1))(*views)
            _lib.check(L.gs_frame_prep_color(cvs, len(views), H, W, self.H_edge, self.W_edge, st), "frame_prep_color")
            if depths:
                dvs = (_lib.DepthView * len(depths))(*depths)
                _lib.check(L.gs_frame_prep_depth(dvs, len(depths), float(self.png_depth_scale), H, W, self.H_edge,
                                                 self.W_edge, st), "frame_prep_depth")
            out = []
            for index, color, d_out in items:
                if self.output == "host":
                    color_h = torch.empty(color.shape, dtype=torch.float32, pin_memory=True)
                    color_h.copy_(color, non_blocking=True)
                    self.bytes_d2h += color.numel() * 4
                    if d_out is not None:
                        depth_h = torch.empty(d_out.shape, dtype=torch.float32, pin_memory=True)
                        depth_h.copy_(d_out, non_blocking=True)
                        self.bytes_d2h += d_out.numel() * 4
                        d_out = depth_h
                    color = color_h
                out.append((index, color, d_out))
            ev = torch.cuda.Event()
            ev.record(side)
        result = []
        for index, color, d_out in out:
            info_pose = None if self.poses is None else torch.from_numpy(self.poses[index]).float()
            result.append(((index, color, d_out, self.intrinsic(), info_pose), ev))
        if self.output == "device":
            # the consumer's stream waits for the side stream, and the side stream's blocks stay reserved until the
            # consumer's work on them is done
            consumer = torch.cuda.current_stream(dev)
            consumer.wait_event(ev)
            for (_, color, d_out, _, _), _ in result:
                color.record_stream(consumer)
                if d_out is not None:
                    d_out.record_stream(consumer)
        return result

    @staticmethod
    def _finish(item, ev):
        ev.synchronize()
        return item


class _Prefetcher:
    """In-order iterator over a dataset: decoder threads run up to a few batches ahead, each batch is enqueued on the
    side stream as soon as it is decoded, and a host item is handed out once its batch's event has completed."""

    def __init__(self, ds):
        self.ds = ds
        self.n = len(ds)
        self.pool = ThreadPoolExecutor(max_workers=max(1, ds.decode_threads), thread_name_prefix="frame-decode")
        self.pending = collections.deque()      # (index, future) in order
        self.ready = collections.deque()        # (item, event)
        self.next_submit = 0
        self.ahead = max(2 * ds.batch, 2 * ds.decode_threads)

    def __iter__(self):
        return self

    def _submit(self):
        while self.next_submit < self.n and len(self.pending) < self.ahead:
            i = self.next_submit
            self.pending.append((i, self.pool.submit(self.ds.decode, i)))
            self.next_submit += 1

    def _launch(self, block):
        batch = []
        while self.pending and len(batch) < self.ds.batch:
            i, fut = self.pending[0]
            if not block and not fut.done():
                break
            self.pending.popleft()
            batch.append((i, fut.result()))
        if batch:
            self.ready.extend(self.ds._prep(batch))
        self._submit()
        return bool(batch)

    def __next__(self):
        self._submit()
        if not self.ready:
            if not self.pending:
                self.close()
                raise StopIteration
            self._launch(block=True)
        # keep the next batch in flight when its frames are already decoded
        if len(self.ready) < self.ds.batch and self.pending and self.pending[0][1].done():
            self._launch(block=False)
        item, ev = self.ready.popleft()
        return item if self.ds.output == "device" else BaseDataset._finish(item, ev)

    def close(self):
        self.pool.shutdown(wait=False, cancel_futures=True)

    def __del__(self):
        try:
            self.close()
        except Exception:       # noqa: BLE001 -- interpreter shutdown
            pass


# ---------------------------------------------------------------------------------------------------- readers ----

class Replica(BaseDataset):
    def __init__(self, cfg, args, device='cuda:0', **options):
        super().__init__(cfg, args, device, **options)
        stride = cfg['stride']
        colors = sorted(glob.glob(f'{self.input_folder}/results/frame*.jpg'))
        depths = sorted(glob.glob(f'{self.input_folder}/results/depth*.png'))
        with open(f'{self.input_folder}/traj.txt', "r") as f:
            lines = f.readlines()
        poses = [np.array(list(map(float, lines[i].split()))).reshape(4, 4) for i in range(len(colors))]
        self.color_paths, self.depth_paths, self.poses = colors[::stride], depths[::stride], poses[::stride]
        self.n_img = len(self.color_paths)


class Azure(BaseDataset):
    def __init__(self, cfg, args, device='cuda:0', **options):
        super().__init__(cfg, args, device, **options)
        self.color_paths = sorted(glob.glob(os.path.join(self.input_folder, 'color', '*.jpg')))
        self.depth_paths = sorted(glob.glob(os.path.join(self.input_folder, 'depth', '*.png')))
        self.n_img = len(self.color_paths)
        log = os.path.join(self.input_folder, 'scene', 'trajectory.log')
        self.poses = []
        if os.path.exists(log):
            with open(log) as f:
                content = f.readlines()
            # blocks of five lines: "src tgt fitness", then the 4x4 matrix
            for i in range(0, len(content), 5):
                values = list(map(float, ''.join(content[i + 1:i + 5]).strip().split()))
                self.poses.append(np.array(values).reshape(4, 4))
        else:
            # the reference sizes this list before it counts the frames, which leaves it empty; identity per frame
            # is what it means
            self.poses = [np.eye(4) for _ in range(self.n_img)]


class ScanNet(BaseDataset):
    def __init__(self, cfg, args, device='cuda:0', **options):
        super().__init__(cfg, args, device, **options)
        stride = cfg['stride']
        max_frames = args.max_frames if args.max_frames >= 0 else int(1e5)
        colors = _numeric_sorted(glob.glob(os.path.join(self.input_folder, 'color', '*.jpg')))
        depths = _numeric_sorted(glob.glob(os.path.join(self.input_folder, 'depth', '*.png')))
        poses = []
        for pose_path in _numeric_sorted(glob.glob(os.path.join(self.input_folder, 'pose', '*.txt'))):
            with open(pose_path, "r") as f:
                poses.append(np.array([list(map(float, line.split(' '))) for line in f.readlines()]).reshape(4, 4))
        self.color_paths = colors[:max_frames][::stride]
        self.depth_paths = depths[:max_frames][::stride]
        self.poses = poses[:max_frames][::stride]
        self.n_img = len(self.color_paths)
        print("INFO: {} images got!".format(self.n_img))


class CoFusion(BaseDataset):
    def __init__(self, cfg, args, device='cuda:0', **options):
        raise NotImplementedError("CoFusion: its depth is EXR (depth_noise/*.exr) and no EXR reader is available here")


class TUM_RGBD(BaseDataset):
    def __init__(self, cfg, args, device='cuda:0', **options):
        super().__init__(cfg, args, device, **options)
        self.color_paths, self.depth_paths, self.poses = self.loadtum(self.input_folder, frame_rate=32)
        self.n_img = len(self.color_paths)

    @staticmethod
    def loadtum(datapath, frame_rate=-1):
        pose_list = _find_pose_list(datapath)
        if pose_list is None:
            raise FileNotFoundError(f"{datapath}: neither groundtruth.txt nor pose.txt")
        image_data = parse_list(os.path.join(datapath, 'rgb.txt'))
        depth_data = parse_list(os.path.join(datapath, 'depth.txt'))
        pose_data = parse_list(pose_list, skiprows=1)
        pose_vecs = pose_data[:, 1:].astype(np.float64)
        tstamp_image = image_data[:, 0].astype(np.float64)
        tstamp_depth = depth_data[:, 0].astype(np.float64)
        tstamp_pose = pose_data[:, 0].astype(np.float64)
        assoc = associate(tstamp_image, tstamp_depth, tstamp_pose)
        # thin to frame_rate: keep an association when its image is more than 1 / frame_rate after the last kept one
        keep = [0]
        for a in range(1, len(assoc)):
            if tstamp_image[assoc[a][0]] - tstamp_image[assoc[keep[-1]][0]] > 1.0 / frame_rate:
                keep.append(a)
        chosen = [assoc[a] for a in keep]
        images = [os.path.join(datapath, image_data[i, 1]) for i, _, _ in chosen]
        depths = [os.path.join(datapath, depth_data[j, 1]) for _, j, _ in chosen]
        return images, depths, relative_poses([pose_vecs[k] for _, _, k in chosen])


class ETH3D(BaseDataset):
    def __init__(self, cfg, args, device='cuda:0', **options):
        super().__init__(cfg, args, device, **options)
        stride = cfg['stride']
        colors, depths, poses, stamps = self.loadtum(self.input_folder)
        self.color_paths, self.depth_paths = colors[::stride], depths[::stride]
        self.poses = None if poses is None else poses[::stride]
        self.image_timestamps = stamps[::stride]
        self.n_img = len(self.color_paths)

    @staticmethod
    def loadtum(datapath):
        pose_list = _find_pose_list(datapath)
        image_data = parse_list(os.path.join(datapath, 'rgb.txt'))
        depth_data = parse_list(os.path.join(datapath, 'depth.txt'))
        tstamp_image = image_data[:, 0].astype(np.float64)
        tstamp_depth = depth_data[:, 0].astype(np.float64)
        if pose_list is None:
            # every image is kept (the benchmark needs a pose for each), paired with its nearest depth
            assoc = associate(tstamp_image, tstamp_depth, None, require_depth=False)
            assert len(assoc) == len(tstamp_image), "Not all images are loaded. While benchmark need all images' pose!"
            print('\nDataset: no gt pose avaliable, {} images found\n'.format(len(tstamp_image)))
            poses = None
        else:
            pose_data = parse_list(pose_list, skiprows=1)
            pose_vecs = pose_data[:, 1:].astype(np.float64)
            assoc = associate(tstamp_image, tstamp_depth, pose_data[:, 0].astype(np.float64))
            poses = relative_poses([pose_vecs[a[2]] for a in assoc])
        images = [os.path.join(datapath, image_data[a[0], 1]) for a in assoc]
        depths = [os.path.join(datapath, depth_data[a[1], 1]) for a in assoc]
        return images, depths, poses, tstamp_image


class EuRoC(BaseDataset):
    def __init__(self, cfg, args, device='cuda:0', **options):
        super().__init__(cfg, args, device, **options)
        stride = cfg['stride']
        left, right, poses = self.loadtum(self.input_folder)
        self.color_paths, self.right_color_paths = left[::stride], right[::stride]
        self.poses = poses[::stride]
        self.n_img = len(self.color_paths)
        self._maps = None

    @staticmethod
    def loadtum(datapath):
        scene_name = datapath.split('/')[-1]
        pose_list = os.path.join(datapath, f'{scene_name}.txt')
        if not os.path.isfile(pose_list):
            raise ValueError(f'EuRoC_DATA_ROOT/{scene_name}/{scene_name}.txt doesn\'t exist!')
        pose_data = parse_list(pose_list, skiprows=1)
        pose_vecs = pose_data[:, 1:].astype(np.float64)
        image_list = sorted(glob.glob(os.path.join(datapath, 'mav0/cam0/data/*.png')))
        tstamp_image = [float(p.split('/')[-1][:-4]) for p in image_list]
        assoc = associate(tstamp_image, None, pose_data[:, 0].astype(np.float64))
        left = [image_list[i] for i, _ in assoc]
        right = [p.replace('cam0', 'cam1') for p in left]
        return left, right, relative_poses([pose_vecs[k] for _, k in assoc])

    def view_paths(self, index):
        paths = [self.color_paths[index]]
        if self.stereo:
            paths.append(self.right_color_paths[index])
        return paths

    def view_maps(self, view, h, w):
        # the rectification maps are EuRoC's own, whatever the decoded size (the reference ignores `distortion` here)
        if self._maps is None:
            self._maps = euroc_maps()
        return self._maps[view]


dataset_dict = {
    "replica": Replica,
    "scannet": ScanNet,
    "cofusion": CoFusion,
    "azure": Azure,
    "tumrgbd": TUM_RGBD,
    'eth3d': ETH3D,
    'euroc': EuRoC,
}
