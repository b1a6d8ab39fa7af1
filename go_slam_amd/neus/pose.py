"""Camera poses as the mapper's bundle adjustment trains them (mapping.BA; reference src/nerf_func.py:44-112): a pose is
the 7-vector [qw, qx, qy, qz, tx, ty, tz] (`Rt_to_quaternion(Tquad=False)`), turned back into a c2w matrix by
`quaternion_to_Rt` -- whose rotation formula scales by 2 / |q|^2 instead of normalising q (the optimiser moves q off the
unit sphere; any nonzero q still gives a rotation).  Plus the HIP reduction of per-ray
gradients to per-pose gradients (gs_pose_grad_reduce)."""
import math

import numpy as np
import torch

from .. import _lib


def rt_to_quaternion(c2w):
    """[4, 4] (or [3, 4]) c2w -> fp32 [7] = [qw, qx, qy, qz, tx, ty, tz] on c2w's device: the unit quaternion of the
    rotation block (Shepperd's method in float64 on the columns normalised first, as mathutils' `to_quaternion` does --
    which of q / -q comes out is immaterial: both give the same matrix, and every AdamW step keeps that true)."""
    dev = c2w.device if torch.is_tensor(c2w) else torch.device("cpu")
    M = (c2w.detach().cpu().double().numpy() if torch.is_tensor(c2w) else np.asarray(c2w, dtype=np.float64))
    R = M[:3, :3] / np.linalg.norm(M[:3, :3], axis=0, keepdims=True)
    t = M[:3, 3]
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr > 0.0:
        s = 2.0 * math.sqrt(1.0 + tr)
        q = [0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s]
    elif R[0, 0] > R[1, 1] and R[0, 0] > R[2, 2]:
        s = 2.0 * math.sqrt(1.0 + R[0, 0] - R[1, 1] - R[2, 2])
        q = [(R[2, 1] - R[1, 2]) / s, 0.25 * s, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s]
    elif R[1, 1] > R[2, 2]:
        s = 2.0 * math.sqrt(1.0 + R[1, 1] - R[0, 0] - R[2, 2])
        q = [(R[0, 2] - R[2, 0]) / s, (R[0, 1] + R[1, 0]) / s, 0.25 * s, (R[1, 2] + R[2, 1]) / s]
    else:
        s = 2.0 * math.sqrt(1.0 + R[2, 2] - R[0, 0] - R[1, 1])
        q = [(R[1, 0] - R[0, 1]) / s, (R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, 0.25 * s]
    q = np.asarray(q) / np.linalg.norm(q)
    return torch.from_numpy(np.concatenate([q, t])).float().to(dev)


def quad2rotation(quad):
    """[B, 4] -> [B, 3, 3]: src/nerf_func.py:44-65 (differentiable; 2 / |q|^2, no normalisation)"""
    qr, qi, qj, qk = quad[:, 0], quad[:, 1], quad[:, 2], quad[:, 3]
    two_s = 2.0 / (quad * quad).sum(-1)
    rows = [
        1 - two_s * (qj ** 2 + qk ** 2), two_s * (qi * qj - qk * qr), two_s * (qi * qk + qj * qr),
        two_s * (qi * qj + qk * qr), 1 - two_s * (qi ** 2 + qk ** 2), two_s * (qj * qk - qi * qr),
        two_s * (qi * qk - qj * qr), two_s * (qj * qk + qi * qr), 1 - two_s * (qi ** 2 + qj ** 2),
    ]
    return torch.stack(rows, -1).reshape(-1, 3, 3)


def quaternion_to_rt(quad_t):
    """[7] or [B, 7] -> [4, 4] or [B, 4, 4] c2w (src/nerf_func.py:91-112), differentiable in quad_t"""
    one = quad_t.dim() == 1
    q = quad_t[None] if one else quad_t
    R = quad2rotation(q[:, :4])
    Rt = torch.cat([R, q[:, 4:, None]], dim=2)
    bottom = torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=q.dtype, device=q.device).expand(q.shape[0], 1, 4)
    Rt = torch.cat([Rt, bottom], dim=1)
    return Rt[0] if one else Rt


def pose_gradients(ray_grad, dirs, seg):
    """Per visit-list entry e, whose rays [seg[e], seg[e+1]) were built as rays_d = dirs @ R_e^T, rays_o = t_e:
    (dL/dR [F, 3, 3], dL/dt [F, 3]) from the per-ray gradients `ray_grad` fp32 [N, 6] = [dL/d rays_o | dL/d rays_d]
    and the camera-frame directions `dirs` fp32 [N, 3].  `seg`: int32 device tensor [F + 1].  One HIP launch, fixed
    summation order (bitwise reproducible)."""
    dev = ray_grad.device
    F = seg.numel() - 1
    assert ray_grad.dtype == torch.float32 and dirs.dtype == torch.float32 and seg.dtype == torch.int32
    assert ray_grad.is_contiguous() and dirs.is_contiguous() and seg.is_contiguous()
    assert ray_grad.shape[1] == 6 and dirs.shape == (ray_grad.shape[0], 3) and seg.device == dev
    out = torch.empty(max(F, 0), 12, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().gs_pose_grad_reduce(_lib.ptr(ray_grad), _lib.ptr(dirs), _lib.ptr(seg), F, _lib.ptr(out),
                                                  _lib.stream_ptr(dev)), "pose_gradients")
    return out[:, :9].reshape(-1, 3, 3), out[:, 9:]
