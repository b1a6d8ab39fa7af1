"""Two `TSDFVolume`s put together: a second session's map registered to the first one's and fused into it.

csrc/tsdf_merge.hip has the two kernels whose samples are lattice points of another volume instead of pixels.
gs_tsdf_register_system gathers a destination volume D and its analytic gradient at the moved lattice points of a source
volume S and reduces the 6 x 6 Gauss-Newton system of the residual f_D - f_S trunc_S / trunc_D in tsdf_align.hip's fixed
fp64 order; the unchanged gs_tsdf_align_step solves it and moves the transform.  gs_tsdf_merge resamples S at D's
lattice points and folds it into D's running mean with S's weights.  Arithmetic contract: include/goslam_hip.h
(gs_tsdf_register_*, gs_tsdf_merge); tests/tsdf_merge_restatement.py restates it.

`register_volumes` refines given transforms coarse to fine (`TSDFVolume.register`), `merge_volume` fuses one volume into
another in place (`TSDFVolume.merge`), `union_volume` makes the empty volume that encloses several moved ones,
`join_volumes` does all three for a list of volumes, and `merge_text` / `parse_merge` write and read
metrics_tsdf_merge.txt (tsdf.fuse_from_config, cfg["tsdf"]["merge"]).

The basin is the truncation, as for `align`: a start further off than that finds no overlap of the two bands.  Offer a
batch of hypotheses instead; there is no global search here.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from . import localize as _localize

DEFAULT_LEVELS = ((4, 10), (2, 10), (1, 5))      # (lattice stride, Gauss-Newton iterations), coarse to fine
RIGID_TOL = 1e-6                                 # |R^T R - I| a transform may have and still be inverted as rigid


def transforms34(T, what):
    """float64 [B,3,4] (host) from transforms [B,4,4] / [B,3,4] or one [4,4] / [3,4]; ValueError for another shape, a
    non-finite entry or a matrix that is no rotation to RIGID_TOL."""
    try:
        m = _localize.poses34(T, what)
    except ValueError as e:
        raise ValueError(str(e).replace("camera-to-world poses", "transforms").replace("camera-to-world pose",
                                                                                       "transform")) from None
    R = m[:, :, :3]
    if m.shape[0] and (np.abs(R.transpose(0, 2, 1) @ R - np.eye(3)).max() > RIGID_TOL or (np.linalg.det(R) < 0).any()):
        raise ValueError(f"{what}: a transform's 3 x 3 part is no rotation (|R^T R - I| > {RIGID_TOL} or det < 0)")
    return m


def _volume(vol, what, name):
    for attr in ("tsdf", "weight", "dims", "lo", "voxel", "trunc", "device"):
        if not hasattr(vol, attr):
            raise ValueError(f"{what}: {name} is no TSDFVolume (it has no .{attr})")
    return vol


def _lattice_args(vol):
    nx, ny, nz = vol.dims
    return [nx, ny, nz, float(vol.lo[0]), float(vol.lo[1]), float(vol.lo[2]), vol.voxel, vol.trunc]


@torch.no_grad()
def register_volumes(dst, src, T_init, levels=DEFAULT_LEVELS, huber=0.5, min_weight=1.0, lam_rel=1e-6, lam_abs=1e-9,
                     min_count=64):
    """Refine B transforms S-world to D-world so that the surfaces of the volume `src` (S) fall onto those of `dst` (D).
    T_init [B,4,4] / [B,3,4] / [3,4] / [4,4] in fp64, rigid: a batch of hypotheses shares every launch.  levels: (lattice
    stride, iterations) pairs run in order, the samples being S's lattice points with every index a multiple of the
    stride; a sample counts where S was seen `min_weight` times and is unsaturated in both truncations, and is used where
    D's cell under it was seen at all eight corners and is unsaturated; huber in units of D's truncation; a step solves
    (H + lam_rel diag H + lam_abs I) x = -b and is refused (the transform stays) with fewer than min_count samples.

    Every level's system / step pairs and one closing system at the last level's stride are enqueued on the current
    stream; the transforms, the closing rows and the trace are read once.  -> host arrays {"T": float64 [B,4,4], "ok":
    bool [B] (the last step was taken and the closing system has min_count samples), "rmse_m": trunc_D * sqrt(mean r^2)
    over the closing samples (inf without one), "overlap": count / considered, the share of S's usable samples that found
    a usable cell of D, "count", "trace": float64 [iterations,B,4] = (cost, count, considered, status) per step,
    "moved_m", "moved_deg": against T_init (the translation is that of S's origin, about which the step turns),
    "moved_constrained_m", "n_constrained": `localize.constrained_movement` of the translation under the closing system}.
    ValueError for bad arguments, before the library or the device is reached."""
    what = "register_volumes"
    _volume(dst, what, "dst"), _volume(src, what, "src")
    if dst is src:
        raise ValueError(f"{what}: dst and src are the same volume")
    if torch.device(dst.device) != torch.device(src.device):
        raise ValueError(f"{what}: dst is on {dst.device}, src on {src.device}")
    poses = transforms34(T_init, what)
    levels = _localize._levels(levels, what)
    huber, min_weight = float(huber), float(min_weight)
    if not huber > 0:
        raise ValueError(f"{what}: huber must be positive, in units of the destination's truncation (got {huber})")
    if math.isnan(min_weight):
        raise ValueError(f"{what}: min_weight is NaN")
    dev = dst.device

    def workspace_bytes(B, min_stride):
        nbytes = _lib.lib().gs_tsdf_register_workspace_bytes(B, *src.dims, min_stride)
        if B and nbytes == 0:
            raise ValueError(f"{what}: {B} transforms of a {src.dims} lattice are too many for one call")
        return nbytes

    def system(stride, pose, rows, workspace):
        with torch.cuda.device(dev):
            rc = _lib.lib().gs_tsdf_register_system(
                _lib.ptr(dst.tsdf), _lib.ptr(dst.weight), *_lattice_args(dst), _lib.ptr(src.tsdf), _lib.ptr(src.weight),
                *_lattice_args(src), _lib.ptr(pose), int(pose.shape[0]), int(stride), min_weight, huber, _lib.ptr(workspace),
                _lib.ptr(rows), _lib.stream_ptr(dev))
        _lib.check(rc, what)

    res = _localize.gauss_newton(what, dev, poses, levels, dst.trunc, lam_rel, lam_abs, min_count, workspace_bytes,
                                 system)
    res["T"], res["overlap"] = res.pop("matrix"), res.pop("ratio")
    return res


def inverse32(T):
    """float32 [3,4]: the inverse (R^T, -R^T t) of a rigid float64 [3,4] transform, formed in float64 and rounded once."""
    Rt = T[:, :3].T
    return np.ascontiguousarray(np.concatenate([Rt, -(Rt @ T[:, 3:])], 1).astype(np.float32))


@torch.no_grad()
def merge_volume(dst, src, T=None, min_weight=1.0):
    """Fuse the volume `src` into `dst` in place (gs_tsdf_merge): every lattice point of `dst` whose image lies in a cell
    of `src` seen `min_weight` times at all eight corners takes the weighted mean of its value and the trilinear value of
    `src` there, with the trilinear weight of `src`; colours likewise.  T [3,4] / [4,4] fp64 maps src's world to dst's
    (what `register_volumes` returns; None: the identity); its inverse is formed in fp64 and rounded once.  src's
    truncation must be at least dst's.  Drops dst's brick flags, enqueues on the current stream, reads nothing, returns
    dst.  ValueError for bad arguments, before the library or the device is reached."""
    what = "TSDFVolume.merge"
    _volume(dst, what, "self"), _volume(src, what, "other")
    if dst is src:
        raise ValueError(f"{what}: a volume cannot be merged into itself")
    if torch.device(dst.device) != torch.device(src.device):
        raise ValueError(f"{what}: self is on {dst.device}, other on {src.device}")
    if not np.float32(src.trunc) >= np.float32(dst.trunc):
        raise ValueError(f"{what}: the other volume's truncation {src.trunc} is smaller than this one's {dst.trunc}: it "
                         "saturates earlier and knows only \"free\" where this volume wants a distance (merge into a "
                         "volume with the smaller truncation, union_volume's default)")
    min_weight = float(min_weight)
    if not min_weight > 0:
        raise ValueError(f"{what}: min_weight must be positive (got {min_weight})")
    if T is None:
        m = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)
    else:
        m = transforms34(T, what)
        if m.shape[0] != 1:
            raise ValueError(f"{what}: one transform, [3,4] or [4,4] (got {m.shape[0]})")
        m = m[0]
    d2s = inverse32(m)
    color = getattr(dst, "colors", None) is not None and getattr(src, "colors", None) is not None
    dev = dst.device
    L = _lib.lib()
    dst._flags = None
    with torch.cuda.device(dev):
        rc = L.gs_tsdf_merge(_lib.ptr(dst.tsdf), _lib.ptr(dst.weight), _lib.ptr(dst.colors) if color else None,
                             *_lattice_args(dst), dst.max_weight, _lib.ptr(src.tsdf), _lib.ptr(src.weight),
                             _lib.ptr(src.colors) if color else None, *_lattice_args(src),
                             d2s.ctypes.data_as(ctypes.c_void_p), min_weight, _lib.stream_ptr(dev))
    _lib.check(rc, what)
    return dst


def moved_box(vol, T):
    """float64 [8,3]: the corners of `vol`'s box lo .. lo + (n - 1) voxel moved by the [3,4] transform T, in fp64."""
    lo = np.asarray(vol.lo, np.float64)
    hi = lo + (np.asarray(vol.dims, np.float64) - 1.0) * float(vol.voxel)
    corners = np.array([[(lo, hi)[i][0], (lo, hi)[j][1], (lo, hi)[k][2]] for i in (0, 1) for j in (0, 1) for k in (0, 1)])
    return corners @ T[:, :3].T + T[:, 3]


def union_volume(volumes, transforms, voxel_size=None, trunc=None, max_weight=None, device=None):
    """An empty TSDFVolume whose bound encloses every volume's box moved by its transform (volume-world to the union's
    world, [3,4] / [4,4] each or None for the identity; the eight corners are moved in fp64).  voxel_size defaults to the
    smallest of the inputs', trunc to the smallest of their truncations (every input may then be merged into it),
    max_weight to the largest, device to the first volume's.  Passes on `lattice`'s ValueError when an axis would need
    more than 1024 points."""
    from .tsdf import TSDFVolume
    what = "union_volume"
    volumes = list(volumes)
    if not volumes:
        raise ValueError(f"{what}: no volume")
    transforms = [None] * len(volumes) if transforms is None else list(transforms)
    if len(transforms) != len(volumes):
        raise ValueError(f"{what}: {len(transforms)} transforms for {len(volumes)} volumes")
    eye = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)
    corners = []
    for i, (vol, T) in enumerate(zip(volumes, transforms)):
        _volume(vol, what, f"volume {i}")
        if T is None:
            m = eye
        else:
            m = transforms34(T, what)
            if m.shape[0] != 1:
                raise ValueError(f"{what}: transform {i} must be one [3,4] or [4,4] matrix")
            m = m[0]
        corners.append(moved_box(vol, m))
    corners = np.concatenate(corners)
    bound = np.stack([corners.min(0), corners.max(0)], 1)
    voxel = min(float(v.voxel) for v in volumes) if voxel_size is None else float(voxel_size)
    trunc = min(float(v.trunc) for v in volumes) if trunc is None else float(trunc)
    max_weight = max(float(getattr(v, "max_weight", 64.0)) for v in volumes) if max_weight is None else float(max_weight)
    return TSDFVolume(bound, voxel, trunc=trunc, max_weight=max_weight, device=volumes[0].device if device is None else device)


@torch.no_grad()
def join_volumes(volumes, T_inits=None, register=True, voxel_size=None, trunc=None, max_weight=None, device=None,
                 min_weight=1.0, **register_args):
    """One map out of several: every further volume is registered to the first (`register_volumes` from T_inits[i],
    volume i's world to volume 0's; None: the identity; T_inits[0] is ignored), a `union_volume` in volume 0's world is
    made and all volumes are merged into it in order.  register=False takes T_inits as they are.  `register_args`:
    levels, huber, lam_rel, lam_abs, min_count.  -> (the joined TSDFVolume, transforms float64 [n,4,4], a report per
    volume: register_volumes' scalars for that volume plus "registered"; volume 0's is {"registered": False, "ok":
    True}).  ValueError when a registration fails, before a union is made: a failed transform must not reach a map."""
    what = "join_volumes"
    volumes = list(volumes)
    if not volumes:
        raise ValueError(f"{what}: no volume")
    T_inits = [None] * len(volumes) if T_inits is None else list(T_inits)
    if len(T_inits) != len(volumes):
        raise ValueError(f"{what}: {len(T_inits)} transforms for {len(volumes)} volumes")
    transforms = np.tile(np.eye(4), (len(volumes), 1, 1))
    reports = [{"registered": False, "ok": True}]
    for i in range(1, len(volumes)):
        start = transforms34(np.eye(4) if T_inits[i] is None else T_inits[i], what)
        if start.shape[0] != 1:
            raise ValueError(f"{what}: T_inits[{i}] must be one [3,4] or [4,4] matrix")
        if register:
            res = register_volumes(volumes[0], volumes[i], start, min_weight=min_weight, **register_args)
            rep = {k: (res[k][0].item() if k != "T" else res[k][0]) for k in res if k != "trace"}
            rep["registered"] = True
            if not rep["ok"]:
                raise ValueError(f"{what}: the registration of volume {i} failed ({rep['count']} samples, overlap "
                                 f"{rep['overlap']!r}); pass a better T_inits[{i}] or register=False")
            transforms[i] = rep["T"]
        else:
            rep = {"registered": False, "ok": True}
            transforms[i, :3, :] = start[0]
        reports.append(rep)
    joined = union_volume(volumes, list(transforms), voxel_size, trunc, max_weight, device)
    for vol, T in zip(volumes, transforms):
        merge_volume(joined, vol, T, min_weight)
    return joined, transforms, reports


# ---- metrics_tsdf_merge.txt -------------------------------------------------------------------------------------------
MERGE_REPORT_ORDER = ("ok", "registered", "overlap", "rmse_m", "moved_m", "moved_deg", "moved_constrained_m",
                      "n_constrained", "count")
_MERGE_INT = ("ok", "registered", "n_constrained", "count")


def merge_report(rep):
    """The reported dict of one of `join_volumes`' reports: MERGE_REPORT_ORDER's keys, nan / 0 where the volume was not
    registered."""
    out = {}
    for k in MERGE_REPORT_ORDER:
        v = rep.get(k, 0 if k in _MERGE_INT else math.nan)
        out[k] = int(v) if k in _MERGE_INT else float(v)
    return out


def merge_text(result, T):
    """The text of metrics_tsdf_merge.txt: two header lines, `name<TAB>value` per reported value, then the three rows of
    the transform this run's world to the earlier volume's.  Numbers are written with repr(): `parse_merge` gives them
    back bit for bit."""
    T = np.asarray(T, np.float64)[:3, :]
    lines = ["Registration of this run's TSDF volume to an earlier run's and their merge: the share of this volume's "
             "usable lattice points that found a usable cell of the earlier one, the residual rmse [m], how far the "
             "transform moved from its start [m, deg] and how far along the directions the surfaces constrain",
             "(nan and 0 where the transform was taken as given; then the transform this run's world to the earlier "
             "volume's, three rows of r0 r1 r2 t)"]
    lines += [f"{k}\t{result[k]!r}" for k in MERGE_REPORT_ORDER]
    lines += [" ".join(repr(float(v)) for v in row) for row in T]
    return "\n".join(lines) + "\n"


def parse_merge(text):
    """merge_text's inverse: (reported dict, transform float64 [3,4])."""
    lines = text.splitlines()
    if len(lines) != 2 + len(MERGE_REPORT_ORDER) + 3 or not lines[0].startswith("Registration of this run's TSDF volume"):
        raise ValueError("not a metrics_tsdf_merge.txt")
    result = {}
    for key, line in zip(MERGE_REPORT_ORDER, lines[2:]):
        name, value = line.split("\t")
        if name != key:
            raise ValueError(f"metrics_tsdf_merge.txt: expected {key}, found {name}")
        result[key] = int(value) if key in _MERGE_INT else float(value)
    T = np.array([[float(v) for v in line.split(" ")] for line in lines[2 + len(MERGE_REPORT_ORDER):]], np.float64)
    if T.shape != (3, 4):
        raise ValueError("metrics_tsdf_merge.txt: the transform is not three rows of four numbers")
    return result, T
