"""Trajectory evaluation at the end of a run, on the device in fp64 (reference src/slam.py:313-365, which goes through
lietorch on the device, then evo on the host): camera-to-world poses of the filled trajectory (gs_traj_world), the
moments of the Umeyama Sim(3) alignment (gs_ape_moments) and the APE statistics of the translation part
(gs_ape_stats).  The 3x3 SVD between the two, nine numbers, stays in NumPy and follows eval_ate.umeyama_alignment.

Contracts: include/goslam_hip.h; tests/traj_eval_restatement.py restates the kernels on the CPU.
"""
import numpy as np
import torch

from . import _lib

STAT_NAMES = ("rmse", "mean", "median", "min", "max", "sse", "std")     # order of gs_ape_stats' output
REPORT_ORDER = ("max", "mean", "median", "min", "rmse", "sse", "std")   # order of the lines of metrics_traj.txt


def _workspace(n, device):
    nbytes = _lib.lib().gs_traj_eval_workspace_bytes(int(n))
    return torch.empty(nbytes, dtype=torch.uint8, device=device), nbytes


def _dev64(x, device):
    return torch.as_tensor(x, dtype=torch.float64, device=device).contiguous()


def world_poses(w2c, compensate):
    """w2c f32 [N,7] (device), compensate f32 [7]: (tq f64 [N,7], c2w f64 [N,4,4]) of compensate * inv(w2c)."""
    w2c = w2c.detach().to(torch.float32).contiguous()
    if not w2c.is_cuda:
        raise RuntimeError("traj_eval.world_poses needs a GPU tensor (go_slam_amd has no CPU fallback)")
    comp = compensate.detach().to(device=w2c.device, dtype=torch.float32).reshape(7).contiguous()
    n = w2c.shape[0]
    tq = torch.empty(n, 7, dtype=torch.float64, device=w2c.device)
    mat = torch.empty(n, 4, 4, dtype=torch.float64, device=w2c.device)
    _lib.check(_lib.lib().gs_traj_world(_lib.ptr(w2c), _lib.ptr(comp), n, _lib.ptr(tq), _lib.ptr(mat),
                                        _lib.stream_ptr(w2c.device)), "gs_traj_world")
    return tq, mat


def ape_moments(est, ref, mask=None):
    """est, ref f64 [N,3] on the device, mask bool/u8 [N] or None: f64 [17] (count, mean est, mean ref, 3x3
    cross-covariance with ref along the rows, variance of est), on the device."""
    if not est.is_cuda:
        raise RuntimeError("traj_eval.ape_moments needs GPU tensors (go_slam_amd has no CPU fallback)")
    est, ref = _dev64(est, est.device), _dev64(ref, est.device)
    assert est.shape == ref.shape and est.dim() == 2 and est.shape[1] == 3
    n = est.shape[0]
    m8 = None if mask is None else mask.to(device=est.device, dtype=torch.uint8).contiguous()
    out = torch.empty(17, dtype=torch.float64, device=est.device)
    ws, nbytes = _workspace(n, est.device)
    _lib.check(_lib.lib().gs_ape_moments(_lib.ptr(est), _lib.ptr(ref), _lib.ptr(m8), n, _lib.ptr(out), _lib.ptr(ws),
                                         nbytes, _lib.stream_ptr(est.device)), "gs_ape_moments")
    return out


def ape_stats(est, ref, cR, t, mask=None):
    """(err f64 [N], stats f64 [7] in STAT_NAMES order), both on the device, for the similarity x -> cR x + t."""
    if not est.is_cuda:
        raise RuntimeError("traj_eval.ape_stats needs GPU tensors (go_slam_amd has no CPU fallback)")
    est, ref = _dev64(est, est.device), _dev64(ref, est.device)
    n = est.shape[0]
    m8 = None if mask is None else mask.to(device=est.device, dtype=torch.uint8).contiguous()
    sim = torch.from_numpy(np.concatenate([np.asarray(cR, dtype=np.float64).reshape(9),
                                           np.asarray(t, dtype=np.float64).reshape(3)])).to(est.device)
    err = torch.empty(n, dtype=torch.float64, device=est.device)
    stats = torch.empty(7, dtype=torch.float64, device=est.device)
    ws, nbytes = _workspace(n, est.device)
    _lib.check(_lib.lib().gs_ape_stats(_lib.ptr(est), _lib.ptr(ref), _lib.ptr(m8), _lib.ptr(sim), n, _lib.ptr(err),
                                       _lib.ptr(stats), _lib.ptr(ws), nbytes, _lib.stream_ptr(est.device)),
               "gs_ape_stats")
    return err, stats


def umeyama_from_moments(moments, with_scale=True):
    """(R, t, c) from gs_ape_moments' 17 numbers: eval_ate.umeyama_alignment from its SVD on, with its ValueError."""
    m = np.asarray(moments, dtype=np.float64)
    if m[0] < 1:
        raise ValueError("degenerate covariance rank, Umeyama alignment is not possible")
    mx, my, cov, sx = m[1:4], m[4:7], m[7:16].reshape(3, 3), m[16]
    U, D, Vt = np.linalg.svd(cov)
    if np.count_nonzero(D > np.finfo(D.dtype).eps) < 2:
        raise ValueError("degenerate covariance rank, Umeyama alignment is not possible")
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0.0:
        S[2, 2] = -1.0
    R = U @ S @ Vt
    c = float(np.trace(np.diag(D) @ S) / sx) if with_scale else 1.0
    t = my - c * (R @ mx)
    return R, t, c


def ape(est, ref, mask=None, align=True, correct_scale=True):
    """APE of the translation part after Sim(3) Umeyama alignment: a dict with the seven statistics (floats), `count`,
    `rotation`, `translation`, `scale`, `alignment_transformation_sim3` [4,4] and `errors` (device f64 [N], -1 outside
    the mask).  One host read of 17 numbers, one of 7."""
    R, t, c = np.eye(3), np.zeros(3), 1.0
    if align:
        R, t, c = umeyama_from_moments(ape_moments(est, ref, mask).cpu().numpy(), with_scale=correct_scale)
    err, stats = ape_stats(est, ref, c * R, t, mask)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = c * R, t
    out = {k: float(v) for k, v in zip(STAT_NAMES, stats.cpu().tolist())}
    count = int(est.shape[0] if mask is None else mask.to(torch.int64).sum())
    out.update(count=count, rotation=R, translation=t, scale=c, alignment_transformation_sim3=T, errors=err)
    return out


def metrics_text(stats):
    """The text appended to metrics_traj.txt: a two-line header and one `name<TAB>value` line per statistic.  The values
    are written with repr(), so reading the file gives back the fp64 numbers bit for bit."""
    lines = ["APE w.r.t. translation part (m)", "(with Sim(3) Umeyama alignment, scale corrected)"]
    lines += [f"{k}\t{float(stats[k])!r}" for k in REPORT_ORDER]
    return "\n".join(lines) + "\n"
