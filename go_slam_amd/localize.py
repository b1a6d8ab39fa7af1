"""Where is this camera in the volume that is already there?  Depth images aligned to a fused `TSDFVolume`.

csrc/tsdf_align.hip minimises the sum of squared TSDF values at a depth image's back-projected pixels over the six pose
parameters (direct SDF alignment: no data association, no raycast, no neighbour search): gs_tsdf_align_system gathers the
TSDF and its analytic gradient and reduces the 6 x 6 Gauss-Newton system in a fixed fp64 order, gs_tsdf_align_step solves
it and moves the pose.  Arithmetic contract: include/goslam_hip.h (gs_tsdf_align_*); tests/tsdf_align_restatement.py
restates it.

`align` refines given poses coarse to fine (`TSDFVolume.align`), `pose_scores` only measures how well poses fit
(`TSDFVolume.pose_scores`), `candidate_poses` and `relocalize` find a pose without a prior among given standpoints,
`save_volume` / `load_volume` carry a volume from one run to the next (`TSDFVolume.save` / `.load`), and `align_stream`
writes metrics_tsdf_align.txt at the end of a run (tsdf.fuse_from_config, cfg["tsdf"]["align"]).
"""
import math

import numpy as np
import torch

from . import _lib

DEFAULT_LEVELS = ((4, 10), (2, 10), (1, 5))      # (pixel stride, Gauss-Newton iterations), coarse to fine
ALIGN_BATCH = 16                                 # frames per `align` call in align_stream


def _host(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def poses34(c2w, what):
    """float64 [B,3,4] (host) from camera-to-world matrices [B,4,4] / [B,3,4] or one [4,4] / [3,4]; ValueError for
    another shape or a non-finite entry."""
    if isinstance(c2w, (list, tuple)) and len(c2w) and np.ndim(_host(c2w[0])) == 2:
        c2w = np.stack([np.asarray(_host(m), dtype=np.float64) for m in c2w])
    m = np.asarray(_host(c2w), dtype=np.float64)
    if m.ndim == 2:
        m = m[None]
    if m.ndim != 3 or tuple(m.shape[1:]) not in ((4, 4), (3, 4)):
        raise ValueError(f"{what}: camera-to-world poses must be [B,4,4] or [B,3,4] (got {list(m.shape)})")
    if not np.isfinite(m).all():
        raise ValueError(f"{what}: a camera-to-world pose holds a non-finite entry")
    return np.ascontiguousarray(m[:, :3, :])


def _levels(levels, what):
    try:
        out = [(int(s), int(n)) for s, n in levels]
        same = all(float(s) == int(s) and float(n) == int(n) for s, n in levels)
    except (TypeError, ValueError):
        out, same = [], False
    if not out or not same or any(s < 1 or n < 0 for s, n in out):
        raise ValueError(f"{what}: levels must be a non-empty list of (stride >= 1, iterations >= 0) integer pairs "
                         f"(got {levels!r})")
    return out


def _inputs(vol, what, depth, c2w, intrinsics, frame, huber, max_depth, min_weight):
    """Everything `align` and `pose_scores` share, checked on the host before the library or the device is reached: ->
    (depth [k,H,W] where it was, poses float64 [B,3,4] host, frame int32 [B] host, [fx, fy, cx, cy], huber, max_depth,
    min_weight)."""
    depth = torch.as_tensor(depth)
    if depth.dim() == 2:
        depth = depth[None]
    if depth.dim() != 3 or min(depth.shape) < 1:
        raise ValueError(f"{what}: depth must be [k,H,W] or [H,W] with k, H, W >= 1 (got {list(depth.shape)})")
    k, H, W = (int(s) for s in depth.shape)
    if H * W > 2 ** 30:
        raise ValueError(f"{what}: {H} x {W} pixels, at most 2^30")
    poses = poses34(c2w, what)
    B = poses.shape[0]
    if frame is None:
        if B != k:
            raise ValueError(f"{what}: {B} poses for {k} depth maps (pass frame=[...] to say which map a pose looks at)")
        fr = np.arange(B, dtype=np.int32)
    else:
        f = _host(frame)
        if f.ndim != 1 or f.shape[0] != B or not (np.issubdtype(f.dtype, np.integer) and f.dtype != np.bool_):
            raise ValueError(f"{what}: frame must be {B} integers, one per pose (got {f.dtype} {list(f.shape)})")
        if B and (f.min() < 0 or f.max() >= k):
            raise ValueError(f"{what}: frame values must lie in [0, {k}) (got {int(f.min())} .. {int(f.max())})")
        fr = f.astype(np.int32)
    intr = list(intrinsics) if isinstance(intrinsics, (tuple, list)) else _host(intrinsics).reshape(-1).tolist()
    if len(intr) != 4:
        raise ValueError(f"{what}: intrinsics must be (fx, fy, cx, cy)")
    intr = [float(v) for v in intr]
    if not all(math.isfinite(v) for v in intr) or intr[0] == 0 or intr[1] == 0:
        raise ValueError(f"{what}: intrinsics must be finite with fx, fy != 0 (got {intr})")
    huber, max_depth, min_weight = float(huber), float(max_depth), float(min_weight)
    if not huber > 0:
        raise ValueError(f"{what}: huber must be positive, in units of the truncation (got {huber})")
    if not max_depth > 0:
        raise ValueError(f"{what}: max_depth must be positive; inf keeps every depth (got {max_depth})")
    if math.isnan(min_weight):
        raise ValueError(f"{what}: min_weight is NaN")
    return depth, poses, fr, intr, huber, max_depth, min_weight


def _buffers(dev, poses, nbytes):
    """(pose [B,3,4], rows [B,32], the chunks' workspace of `nbytes`): float64 on `dev`."""
    B = int(poses.shape[0])
    return (torch.from_numpy(poses).to(dev), torch.empty(B, 32, dtype=torch.float64, device=dev),
            torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=dev))


class _Systems:
    """gs_tsdf_align_system for poses against depth maps.  The depth maps and the poses' frames go to the device at the
    first `system`, which enqueues on the current stream and reads nothing."""

    def __init__(self, vol, depth, frame, intr, huber, max_depth, min_weight, what):
        self.vol, self.intr, self.what = vol, intr, what
        self.depth, self.frame, self.on_device = depth, frame, None
        self.huber, self.max_depth, self.min_weight = huber, max_depth, min_weight

    def workspace_bytes(self, B, min_stride):
        k, H, W = self.depth.shape
        nbytes = _lib.lib().gs_tsdf_align_workspace_bytes(B, H, W, min_stride)
        if B and nbytes == 0:
            raise ValueError(f"{self.what}: {B} poses of {H} x {W} pixels at stride {min_stride} are too many for one call")
        return nbytes

    def system(self, stride, pose, rows, workspace):
        vol = self.vol
        if self.on_device is None:
            self.on_device = (self.depth.to(device=vol.device, dtype=torch.float32).contiguous(),
                              torch.from_numpy(self.frame).to(vol.device))
        depth, frame = self.on_device
        nx, ny, nz = vol.dims
        k, H, W = depth.shape
        with torch.cuda.device(vol.device):
            rc = _lib.lib().gs_tsdf_align_system(
                _lib.ptr(vol.tsdf), _lib.ptr(vol.weight), nx, ny, nz, _lib.ptr(depth), _lib.ptr(frame), _lib.ptr(pose),
                int(pose.shape[0]), int(k), int(H), int(W), int(stride), *self.intr, float(vol.lo[0]), float(vol.lo[1]),
                float(vol.lo[2]), vol.voxel, self.max_depth, self.min_weight, self.huber, _lib.ptr(workspace),
                _lib.ptr(rows), _lib.stream_ptr(vol.device))
        _lib.check(rc, self.what)


def gauss_newton(what, dev, poses, levels, trunc, lam_rel, lam_abs, min_count, workspace_bytes, system):
    """The coarse-to-fine Gauss-Newton run that `align` and `tsdf_merge.register_volumes` are, from host poses float64
    [B,3,4] and checked `levels`.  workspace_bytes(B, min_stride) gives the size of the chunks' workspace at the smallest
    stride (and raises the caller's ValueError when there is none); system(stride, pose, rows, workspace) enqueues the
    caller's system for the device poses.  Every level's system / gs_tsdf_align_step pairs and one closing system at the
    last level's stride are enqueued on the current stream; poses, closing rows and trace are read once.  -> the result
    both callers document, with the final [B,4,4] matrices as "matrix" and count / considered as "ratio" (a caller gives
    the two its own names) and rmse_m = trunc * sqrt(sq / count).  ValueError for bad lam_rel, lam_abs or min_count,
    before the library or the device is reached."""
    lam_rel, lam_abs = float(lam_rel), float(lam_abs)
    if not (0 <= lam_rel < math.inf and 0 <= lam_abs < math.inf):
        raise ValueError(f"{what}: lam_rel and lam_abs must be finite and >= 0 (got {lam_rel}, {lam_abs})")
    if isinstance(min_count, bool) or int(min_count) != min_count or int(min_count) < 1:
        raise ValueError(f"{what}: min_count must be an integer >= 1 (got {min_count!r})")
    min_count = int(min_count)
    B = int(poses.shape[0])
    iters = sum(n for _, n in levels)
    pose, rows, workspace = _buffers(dev, poses, workspace_bytes(B, min(s for s, _ in levels)))
    trace = torch.zeros(iters, B, 4, dtype=torch.float64, device=dev)
    it = 0
    for stride, n in levels:
        for _ in range(n):
            system(stride, pose, rows, workspace)
            with torch.cuda.device(dev):
                rc = _lib.lib().gs_tsdf_align_step(_lib.ptr(rows), _lib.ptr(pose), B, lam_rel, lam_abs, min_count,
                                                   _lib.ptr(trace[it]), _lib.stream_ptr(dev))
            _lib.check(rc, what)
            it += 1
    system(levels[-1][0], pose, rows, workspace)
    host = torch.cat([pose.reshape(-1), rows.reshape(-1), trace.reshape(-1)]).cpu().numpy()                # the one read
    final = host[:B * 12].reshape(B, 3, 4)
    closing = host[B * 12:B * 44].reshape(B, 32)
    tr = host[B * 44:].reshape(iters, B, 4)
    rmse, share, count = _fit(closing, trunc)
    T = np.zeros((B, 4, 4), np.float64)
    T[:, :3, :] = final
    T[:, 3, 3] = 1.0
    stepped = tr[-1, :, 3] == 1.0 if iters else np.ones(B, bool)
    moved = final[:, :, 3] - poses[:, :, 3]
    constrained_m, n_constrained = constrained_movement(closing, moved)
    return {"matrix": T, "ok": stepped & (count >= min_count), "rmse_m": rmse, "ratio": share, "count": count, "trace": tr,
            "moved_m": np.linalg.norm(moved, axis=1), "moved_deg": rotation_angle_deg(final[:, :, :3], poses[:, :, :3]),
            "moved_constrained_m": constrained_m, "n_constrained": n_constrained}


def _fit(rows, trunc):
    """(rmse_m, inlier_fraction, count) from host rows [B,32]: trunc * sqrt(sq / count), inf without a sample;
    count / considered, 0 without a considered pixel."""
    count, sq, considered = rows[:, 28], rows[:, 29], rows[:, 30]
    with np.errstate(divide="ignore", invalid="ignore"):
        rmse = np.where(count > 0, trunc * np.sqrt(sq / count), np.inf)
        inlier = np.where(considered > 0, count / considered, 0.0)
    return rmse, inlier, count.astype(np.int64)


def rotation_angle_deg(Ra, Rb):
    """The angle between rotations [...,3,3] in degrees, from |Ra - Rb|_F = 2 sqrt(2) sin(theta / 2): no cancellation
    at small angles."""
    s = np.linalg.norm(np.asarray(Ra) - np.asarray(Rb), axis=(-2, -1)) / (2.0 * math.sqrt(2.0))
    return np.degrees(2.0 * np.arcsin(np.minimum(s, 1.0)))


@torch.no_grad()
def align(vol, depth, c2w_init, intrinsics, frame=None, levels=DEFAULT_LEVELS, huber=0.5, max_depth=math.inf,
          min_weight=1.0, lam_rel=1e-6, lam_abs=1e-9, min_count=64):
    """Refine B camera-to-world poses so that the depth images' back-projected pixels fall onto the zero level of `vol`.
    depth [k,H,W] (or [H,W]) in metres, <= 0 or NaN invalid; c2w_init [B,4,4] / [B,3,4]; intrinsics (fx, fy, cx, cy) of
    the depth maps; frame: the depth map each pose looks at (default: pose b looks at map b, B == k).  levels: (pixel
    stride, iterations) pairs run in order; huber in units of the truncation (the residual is the TSDF value); pixels
    deeper than max_depth and cells with a corner seen fewer than min_weight times are left out; a step solves (H +
    lam_rel diag H + lam_abs I) x = -b and is refused (the pose stays) with fewer than min_count samples.

    Every level's system / step pairs and one closing system at the last level's stride are enqueued on the current
    stream; the poses, the closing rows and the trace are read once.  -> host arrays {"c2w": float64 [B,4,4], "ok": bool
    [B] (the last step was taken and the closing system has min_count samples), "rmse_m": trunc * sqrt(mean f^2) over
    the closing samples (inf without one), "inlier_fraction": samples / pixels with depth, "count", "trace": float64
    [iterations,B,4] = (cost, count, considered, status) per step, "moved_m", "moved_deg": against c2w_init,
    "moved_constrained_m", "n_constrained": `constrained_movement` of the translation under the closing system}.
    ValueError for bad arguments, before the library is reached."""
    what = "TSDFVolume.align"
    depth, poses, fr, intr, huber, max_depth, min_weight = _inputs(vol, what, depth, c2w_init, intrinsics, frame, huber,
                                                                   max_depth, min_weight)
    levels = _levels(levels, what)
    sysm = _Systems(vol, depth, fr, intr, huber, max_depth, min_weight, what)
    res = gauss_newton(what, vol.device, poses, levels, vol.trunc, lam_rel, lam_abs, min_count, sysm.workspace_bytes,
                       sysm.system)
    res["c2w"], res["inlier_fraction"] = res.pop("matrix"), res.pop("ratio")
    return res


CONSTRAINED_SHARE = 0.01         # of the largest eigenvalue of H's translation block


def constrained_movement(rows, moved):
    """The part of the translations `moved` [B,3] that the closing systems `rows` [B,32] constrain: (its length [B], the
    number of constrained directions [B]).  H's translation block is sum wt gw gw^T, the weighted scatter of the surface
    gradients the samples saw; a unit direction e has e^T H e = sum wt (gw . e)^2.  An eigen-direction counts as
    constrained when its eigenvalue is at least CONSTRAINED_SHARE of the largest: one surface orientation seen by a
    hundredth of the samples passes, and what noise in the fused gradients puts on a free direction (along a corridor,
    along the edge of two planes) does not.  Along the other directions only the damping holds the pose, and movement
    there says nothing about the pose's error."""
    rows, moved = np.asarray(rows, np.float64).reshape(-1, 32), np.asarray(moved, np.float64).reshape(-1, 3)
    H = np.zeros((rows.shape[0], 3, 3))
    for (i, j), at in (((0, 0), 0), ((0, 1), 1), ((0, 2), 2), ((1, 1), 6), ((1, 2), 7), ((2, 2), 11)):
        H[:, i, j] = H[:, j, i] = rows[:, at]
    w, V = np.linalg.eigh(H)                                                   # ascending eigenvalues, columns of V
    keep = (w >= CONSTRAINED_SHARE * w[:, -1:]) & (w > 0)
    along = np.einsum("bij,bi->bj", V, moved)
    return np.sqrt((along ** 2 * keep).sum(axis=1)), keep.sum(axis=1).astype(np.int64)


@torch.no_grad()
def pose_scores(vol, depth, c2w, intrinsics, frame=None, stride=4, huber=0.5, max_depth=math.inf, min_weight=1.0):
    """How well B poses explain the depth images, without moving them: one system per pose at `stride`, one read.
    Arguments as `align`.  -> host arrays {"rmse_m", "inlier_fraction", "count"} ([B] each)."""
    what = "TSDFVolume.pose_scores"
    depth, poses, fr, intr, huber, max_depth, min_weight = _inputs(vol, what, depth, c2w, intrinsics, frame, huber,
                                                                   max_depth, min_weight)
    if isinstance(stride, bool) or int(stride) != stride or int(stride) < 1:
        raise ValueError(f"{what}: stride must be an integer >= 1 (got {stride!r})")
    stride = int(stride)
    sysm = _Systems(vol, depth, fr, intr, huber, max_depth, min_weight, what)
    pose, rows, workspace = _buffers(vol.device, poses, sysm.workspace_bytes(int(poses.shape[0]), stride))
    sysm.system(stride, pose, rows, workspace)
    rmse, inlier, count = _fit(rows.cpu().numpy(), vol.trunc)                                              # the one read
    return {"rmse_m": rmse, "inlier_fraction": inlier, "count": count}


def candidate_poses(centres, n_yaw, up_axis, pitch=0.0, up_sign=1):
    """float64 [N * n_yaw, 4, 4] camera-to-world matrices (host; candidate c * n_yaw + j): at each world point of
    `centres` [N,3] a camera at the headings 2 pi j / n_yaw about `up_axis`, pitched up by `pitch` radians, without
    roll.  The heading is `view.ray_directions`': yaw 0 looks along the lower of the two other axes and positive yaw
    turns toward the higher one, so the world points of `ESDF.view_candidates`' cells (lo + cell * voxel) can be fed
    here.  The image's y axis points against `up_sign` * up_axis (down, as a sensor's does; up_sign = -1 for a world
    whose up_axis coordinate grows downward) and x = y cross z: a proper rotation for every up_axis."""
    what = "candidate_poses"
    c = np.asarray(_host(centres), dtype=np.float64)
    if c.size == 0:
        c = c.reshape(0, 3)
    if c.ndim != 2 or c.shape[1] != 3 or not np.isfinite(c).all():
        raise ValueError(f"{what}: centres must be finite world points [N,3] (got {list(c.shape)})")
    if isinstance(n_yaw, bool) or int(n_yaw) != n_yaw or int(n_yaw) < 1:
        raise ValueError(f"{what}: n_yaw must be an integer >= 1 (got {n_yaw!r})")
    if isinstance(up_axis, bool) or up_axis not in (0, 1, 2):
        raise ValueError(f"{what}: up_axis must be 0, 1 or 2 (got {up_axis!r})")
    if up_sign not in (1, -1):
        raise ValueError(f"{what}: up_sign must be 1 or -1 (got {up_sign!r})")
    pitch = float(pitch)
    if not math.isfinite(pitch):
        raise ValueError(f"{what}: pitch must be finite (got {pitch!r})")
    up = int(up_axis)
    fwd, left = [a for a in range(3) if a != up]
    out = np.zeros((c.shape[0], int(n_yaw), 4, 4), np.float64)
    for j in range(int(n_yaw)):
        yaw = 2.0 * math.pi * j / int(n_yaw)
        z, u = np.zeros(3), np.zeros(3)
        z[fwd], z[left], z[up] = math.cos(pitch) * math.cos(yaw), math.cos(pitch) * math.sin(yaw), up_sign * math.sin(pitch)
        u[fwd], u[left], u[up] = -math.sin(pitch) * math.cos(yaw), -math.sin(pitch) * math.sin(yaw), up_sign * math.cos(pitch)
        y = -u
        out[:, j, :3, 0], out[:, j, :3, 1], out[:, j, :3, 2] = np.cross(y, z), y, z
    out[:, :, :3, 3] = c[:, None, :]
    out[:, :, 3, 3] = 1.0
    return out.reshape(-1, 4, 4)


def _ranking(passes, rmse):
    """Indices by (passes first, lower rmse, lower index)."""
    return sorted(range(len(rmse)), key=lambda i: (not bool(passes[i]), float(rmse[i]), i))


@torch.no_grad()
def relocalize(vol, depth, intrinsics, candidates, keep=8, min_inlier_fraction=0.5, stride=4, **align_args):
    """Find the pose of one depth image [H,W] in `vol` among `candidates` ([C,4,4] / [C,3,4] camera-to-world, for
    example `candidate_poses`): `pose_scores` of every candidate at `stride`, the `keep` best by (inlier_fraction >=
    min_inlier_fraction first, then the lower rmse, then the lower index) aligned in one `align` batch (`align_args`:
    levels, huber, max_depth, min_weight, lam_rel, lam_abs, min_count), and those ranked again the same way, a pose
    whose alignment is not `ok` counting as failing the threshold.  -> {"found": the best passes, "index": its
    candidate, "c2w": float64 [4,4], "rmse_m", "inlier_fraction", "ranked": the aligned candidates best first as dicts
    (index, c2w, rmse_m, inlier_fraction, ok: the runners-up follow the winner), "scores": pose_scores' dict}; with
    "found" False the other values still describe the best of what there was (index None without candidates)."""
    what = "relocalize"
    depth = torch.as_tensor(depth)
    if depth.dim() == 3 and depth.shape[0] == 1:
        depth = depth[0]
    if depth.dim() != 2:
        raise ValueError(f"{what}: depth must be one image [H,W] (got {list(depth.shape)})")
    cand = poses34(candidates, what) if len(candidates) else np.zeros((0, 3, 4))
    if isinstance(keep, bool) or int(keep) != keep or int(keep) < 1:
        raise ValueError(f"{what}: keep must be an integer >= 1 (got {keep!r})")
    thr = float(min_inlier_fraction)
    if math.isnan(thr):
        raise ValueError(f"{what}: min_inlier_fraction is NaN")
    scoring = {k: align_args[k] for k in ("huber", "max_depth", "min_weight") if k in align_args}
    C = cand.shape[0]
    none = {"found": False, "index": None, "c2w": None, "rmse_m": math.inf, "inlier_fraction": 0.0, "ranked": [],
            "scores": {"rmse_m": np.zeros(0), "inlier_fraction": np.zeros(0), "count": np.zeros(0, np.int64)}}
    if C == 0:
        return none
    zeros = np.zeros(C, np.int32)
    scores = pose_scores(vol, depth, cand, intrinsics, frame=zeros, stride=stride, **scoring)
    kept = _ranking(scores["inlier_fraction"] >= thr, scores["rmse_m"])[:int(keep)]
    res = align(vol, depth, cand[kept], intrinsics, frame=zeros[:len(kept)], **align_args)
    passes = res["ok"] & (res["inlier_fraction"] >= thr)
    ranked = [{"index": kept[i], "c2w": res["c2w"][i], "rmse_m": float(res["rmse_m"][i]),
               "inlier_fraction": float(res["inlier_fraction"][i]), "ok": bool(res["ok"][i])}
              for i in _ranking(passes, res["rmse_m"])]
    best = ranked[0]
    return {"found": bool(best["ok"] and best["inlier_fraction"] >= thr), "index": best["index"], "c2w": best["c2w"],
            "rmse_m": best["rmse_m"], "inlier_fraction": best["inlier_fraction"], "ranked": ranked, "scores": scores}


# ---- a volume on disk -----------------------------------------------------------------------------------------------
VOLUME_KEYS = ("tsdf", "weight", "colors", "lo", "voxel", "trunc", "max_weight", "dims")


def save_volume(vol, path):
    """One .npz with tsdf, weight float32 [nx,ny,nz], colors float32 [3,nx,ny,nz], lo float64 [3], voxel, trunc,
    max_weight float64 and dims int64 [3]; `load_volume` gives the same bits back."""
    with open(path, "wb") as fh:
        np.savez(fh, tsdf=vol.tsdf.cpu().numpy(), weight=vol.weight.cpu().numpy(), colors=vol.colors.cpu().numpy(),
                 lo=np.asarray(vol.lo, np.float64), voxel=np.float64(vol.voxel), trunc=np.float64(vol.trunc),
                 max_weight=np.float64(vol.max_weight), dims=np.asarray(vol.dims, np.int64))


def load_volume(cls, path, device=None):
    """save_volume's inverse as an instance of `cls` (TSDFVolume) on `device`; ValueError for a file without the keys,
    with arrays that disagree with `dims`, or with values no volume can hold."""
    what = "TSDFVolume.load"
    with np.load(path, allow_pickle=False) as data:
        missing = [k for k in VOLUME_KEYS if k not in data.files]
        if missing:
            raise ValueError(f"{what}: {path} lacks {missing}")
        arrays = {k: data[k] for k in VOLUME_KEYS}
    dims = arrays["dims"]
    if dims.shape != (3,) or not np.issubdtype(dims.dtype, np.integer) or (dims < 2).any() or (dims > 1024).any():
        raise ValueError(f"{what}: dims must be three integers in [2, 1024] (got {dims!r})")
    dims = tuple(int(n) for n in dims)
    for name, shape in (("tsdf", dims), ("weight", dims), ("colors", (3,) + dims)):
        a = arrays[name]
        if a.dtype != np.float32 or tuple(a.shape) != shape:
            raise ValueError(f"{what}: {name} is {a.dtype} {list(a.shape)}, dims {list(dims)} need float32 {list(shape)}")
    lo = np.asarray(arrays["lo"], np.float64)
    voxel, trunc, max_weight = (float(arrays[k]) for k in ("voxel", "trunc", "max_weight"))
    if lo.shape != (3,) or not np.isfinite(lo).all() or not (0 < voxel < math.inf and 0 < trunc < math.inf
                                                            and max_weight >= 1):
        raise ValueError(f"{what}: lo {lo!r}, voxel {voxel}, trunc {trunc}, max_weight {max_weight} describe no volume")
    vol = cls.__new__(cls)
    vol.voxel, vol.lo, vol.dims, vol.trunc, vol.max_weight = voxel, lo.copy(), dims, trunc, max_weight
    vol.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    vol.tsdf = torch.from_numpy(arrays["tsdf"]).to(vol.device).contiguous()
    vol.weight = torch.from_numpy(arrays["weight"]).to(vol.device).contiguous()
    vol.colors = torch.from_numpy(arrays["colors"]).to(vol.device).contiguous()
    vol._flags = None
    return vol


# ---- metrics_tsdf_align.txt -----------------------------------------------------------------------------------------
ALIGN_REPORT_ORDER = ("moved_mean_m", "moved_max_m", "moved_mean_deg", "moved_max_deg", "moved_constrained_mean_m",
                      "moved_constrained_max_m", "rmse_mean_m", "rmse_max_m", "inlier_fraction_mean",
                      "inlier_fraction_min", "n_underconstrained", "n_failed", "n_frames")
ALIGN_COLUMNS = 7                # moved_m, moved_deg, rmse_m, inlier_fraction, moved_constrained_m, n_constrained, ok


def summarize_align(per_frame):
    """per_frame: rows (moved_m, moved_deg, rmse_m, inlier_fraction, moved_constrained_m, n_constrained, ok).  -> the
    reported dict: means and extremes over the frames whose alignment is ok (nan without one), n_underconstrained those
    of them with fewer than three constrained directions (their moved_m includes drift along a free one;
    moved_constrained_m does not), n_failed the others."""
    rows = np.asarray(per_frame, dtype=np.float64).reshape(-1, ALIGN_COLUMNS)
    good = rows[rows[:, 6] == 1.0]
    stat = (lambda col, fn: float(fn(good[:, col]))) if len(good) else (lambda col, fn: math.nan)
    return {"moved_mean_m": stat(0, np.mean), "moved_max_m": stat(0, np.max), "moved_mean_deg": stat(1, np.mean),
            "moved_max_deg": stat(1, np.max), "moved_constrained_mean_m": stat(4, np.mean),
            "moved_constrained_max_m": stat(4, np.max), "rmse_mean_m": stat(2, np.mean), "rmse_max_m": stat(2, np.max),
            "inlier_fraction_mean": stat(3, np.mean), "inlier_fraction_min": stat(3, np.min),
            "n_underconstrained": int((good[:, 5] < 3).sum()), "n_failed": int(len(rows) - len(good)),
            "n_frames": int(len(rows))}


def align_text(result, frames, per_frame):
    """The text of metrics_tsdf_align.txt: two header lines, `name<TAB>value` per reported value, then one line per
    aligned frame, `index moved_m moved_deg rmse_m inlier_fraction moved_constrained_m n_constrained ok`.  Numbers are
    written with repr(): `parse_align` gives them back bit for bit."""
    lines = ["Alignment of the sensor depth to the fused TSDF volume, from the estimated pose of every aligned frame: how "
             "far the pose moved [m, deg], how far along the directions the surfaces in view constrain, the residual rmse "
             "[m] and the share of the pixels with depth that were used",
             "(means and extremes over the frames whose alignment succeeded, nan without one; then per frame: index "
             "moved_m moved_deg rmse_m inlier_fraction moved_constrained_m n_constrained ok)"]
    lines += [f"{k}\t{result[k]!r}" for k in ALIGN_REPORT_ORDER]
    rows = np.asarray(per_frame, dtype=np.float64).reshape(len(frames), ALIGN_COLUMNS)
    lines += [f"{int(i)} {float(r[0])!r} {float(r[1])!r} {float(r[2])!r} {float(r[3])!r} {float(r[4])!r} {int(r[5])} "
              f"{int(r[6])}" for i, r in zip(frames, rows)]
    return "\n".join(lines) + "\n"


def parse_align(text):
    """align_text's inverse: (reported dict, [(index, moved_m, moved_deg, rmse_m, inlier_fraction, moved_constrained_m,
    n_constrained, ok), ...])."""
    lines = text.splitlines()
    if len(lines) < 2 + len(ALIGN_REPORT_ORDER) or not lines[0].startswith("Alignment of the sensor depth"):
        raise ValueError("not a metrics_tsdf_align.txt")
    result = {}
    for key, line in zip(ALIGN_REPORT_ORDER, lines[2:]):
        name, value = line.split("\t")
        if name != key:
            raise ValueError(f"metrics_tsdf_align.txt: expected {key}, found {name}")
        result[key] = int(value) if key.startswith("n_") else float(value)
    frames = []
    for line in lines[2 + len(ALIGN_REPORT_ORDER):]:
        i, a, b, c, d, e, n, ok = line.split(" ")
        frames.append((int(i), float(a), float(b), float(c), float(d), float(e), int(n), int(ok)))
    return result, frames


@torch.no_grad()
def align_stream(vol, stream, c2w_list, intrinsics, every=5, out_path=None, **align_args):
    """Align every `every`-th frame of `stream` (item[2]: its sensor depth) to `vol` from its camera-to-world pose
    c2w_list[i], ALIGN_BATCH frames per `align` call.  -> summarize_align()'s dict plus `frames` and `per_frame` (host
    fp64 [F,7]: moved_m, moved_deg, rmse_m, inlier_fraction, moved_constrained_m, n_constrained, ok); with `out_path`
    writes align_text() there."""
    every = int(every)
    if every < 1:
        raise ValueError("align_stream: every must be at least 1")
    frames = list(range(0, len(stream), every))
    rows = []
    for a in range(0, len(frames), ALIGN_BATCH):
        ids = frames[a:a + ALIGN_BATCH]
        depth = torch.stack([stream[i][2].to(vol.device, torch.float32) for i in ids])
        res = align(vol, depth, [torch.as_tensor(c2w_list[i]) for i in ids], intrinsics, **align_args)
        rows.append(np.stack([res["moved_m"], res["moved_deg"], res["rmse_m"], res["inlier_fraction"],
                              res["moved_constrained_m"], res["n_constrained"].astype(np.float64),
                              res["ok"].astype(np.float64)], axis=1))
    per_frame = np.concatenate(rows) if rows else np.zeros((0, ALIGN_COLUMNS), np.float64)
    result = summarize_align(per_frame)
    if out_path is not None:
        with open(out_path, "w") as fh:
            fh.write(align_text(result, frames, per_frame))
    result.update(frames=frames, per_frame=per_frame)
    return result
