"""Differentiable CPU restatement of InstantNeuS.forward in the RAYS (test infrastructure for mapping.BA).

oracle/neus_autograd.py::neus_forward_diff with the sample points differentiable: the hash grid's input derivatives are
taken with `grid_encode_diff(..., x_differentiable=True)` (first order d enc / d x, and the mixed second derivatives of
the trilinear interpolation that d sdf / d x carries -- tiny-cuda-nn's backward_input_backward_input), the colour
embedding sin(x B) and the NeuS alpha's true_cos = dirs . g are differentiable in x and dirs, and the in-bound mask is a
constant (as the reference's is).  torch.autograd on this gives dL/d rays_o and dL/d rays_d of the reference's graph
(src/InstantNeuS.py:295-370 with rays that require grad, src/mapping.py:262-283 under enable_ba)."""
import torch

from oracle import neus_autograd as NA, neus_oracle as NO


def neus_forward_rays_diff(rays_o, rays_d, z_vals, dists, P, meta=None):
    meta = meta or NO.grid_meta()
    n, s = z_vals.shape
    z_mid = z_vals + dists / 2.0
    pts = (rays_o[:, None, :] + rays_d[:, None, :] * z_mid[:, :, None]).reshape(-1, 3)
    dirs = rays_d[:, None, :].expand(n, s, 3).reshape(-1, 3)
    mask = NO.in_bound(pts.detach(), P["rt_bound"])
    if mask.float().sum() < 1:
        mask[:100] = True
    pm = pts[mask]
    bound = P["bound"]
    span = bound[:, 1] - bound[:, 0]
    p = (pm - bound[:, 0]) / span * 2.0 - 1.0
    inside = ((p >= -1.0) & (p <= 1.0)).float().detach()
    p = p.clamp(-1.0, 1.0)
    enc, dydx = NA.grid_encode_diff((p + 1) / 2, P["grid"], meta, x_differentiable=True)
    out = torch.cat([p, enc], -1) @ P["sdf_w"].t() + P["sdf_b"]
    g_enc = NA._ste_half(P["sdf_w"][0, 3:])
    grad_m = (P["sdf_w"][0, :3][None] + torch.einsum("ncd,c->nd", dydx, g_enc) / 2) * inside * 2.0 / span
    npts = pts.shape[0]
    sdf = (torch.ones(npts, 1) * 100).index_put((mask,), out[:, :1])
    grads = torch.zeros(npts, 3).index_put((mask,), grad_m)
    inv_s = torch.exp(P["variance"] * 10.0).clip(1e-6, 1e6)
    alpha = NO.get_alpha(sdf, grads, dirs, dists, inv_s)
    emb = torch.sin(pm @ P["color_B"])
    o_rgb = NA._ste_half(torch.sigmoid(NA.mlp_diff(torch.cat([emb, grad_m, out[:, 1:]], 1), P["mlp"])))
    rgb = torch.zeros(npts, 3).index_put((mask,), o_rgb).reshape(n, s, 3)
    sdf = sdf.reshape(n, s)
    alpha = (alpha * mask[:, None]).reshape(n, s)
    grads = grads.reshape(n, s, 3)
    m2 = mask.reshape(n, s)
    weights = alpha * torch.cumprod(torch.cat([torch.ones(n, 1), 1 - alpha + 1e-7], 1), 1)[:, :-1]
    depth = (z_mid * weights).sum(1, keepdim=True)
    gerr = (torch.linalg.norm(grads, ord=2, dim=2) - 1.0) ** 2 * m2
    return {
        "color": (rgb * weights[:, :, None]).sum(1), "depth": depth,
        "depth_variance": ((z_mid - depth) ** 2 * weights).sum(1, keepdim=True),
        "normal": ((grads * weights[:, :, None]) * m2[:, :, None]).sum(1),
        "weight_sum": weights.sum(1, keepdim=True), "sdf": sdf, "z_vals": z_mid,
        "gradient_error": gerr.mean().unsqueeze(0),
    }


def ray_gradients(rays_o, rays_d, z_vals, dists, P, loss_fn):
    """(dL/d rays_o, dL/d rays_d) of loss_fn(outputs) through the restatement (float32, CPU)"""
    o = rays_o.detach().clone().requires_grad_(True)
    d = rays_d.detach().clone().requires_grad_(True)
    loss = loss_fn(neus_forward_rays_diff(o, d, z_vals, dists, P))
    go, gd = torch.autograd.grad(loss, [o, d], allow_unused=True)
    return (torch.zeros_like(o) if go is None else go), (torch.zeros_like(d) if gd is None else gd)


def pose_gradients_fp64(ray_grad, dirs, counts):
    """per entry (dL/dR [F, 3, 3], dL/dt [F, 3]) in float64: rays of entry e are built as dirs @ R_e^T, t_e"""
    g, dc = ray_grad.double(), dirs.double()
    dR, dt, a = [], [], 0
    for c in counts:
        dR.append(g[a:a + c, 3:].t() @ dc[a:a + c])
        dt.append(g[a:a + c, :3].sum(0))
        a += c
    return torch.stack(dR), torch.stack(dt)


def quad2rotation_fp64(q):
    """src/nerf_func.py:44-65 restated in float64 (2 / |q|^2, no normalisation)"""
    q = q.double()
    qr, qi, qj, qk = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    s = 2.0 / (q * q).sum(-1)
    R = torch.empty(q.shape[0], 3, 3, dtype=torch.float64)
    R[:, 0, 0] = 1 - s * (qj ** 2 + qk ** 2)
    R[:, 0, 1] = s * (qi * qj - qk * qr)
    R[:, 0, 2] = s * (qi * qk + qj * qr)
    R[:, 1, 0] = s * (qi * qj + qk * qr)
    R[:, 1, 1] = 1 - s * (qi ** 2 + qk ** 2)
    R[:, 1, 2] = s * (qj * qk - qi * qr)
    R[:, 2, 0] = s * (qi * qk - qj * qr)
    R[:, 2, 1] = s * (qj * qk + qi * qr)
    R[:, 2, 2] = 1 - s * (qi ** 2 + qj ** 2)
    return R


def fixture_first_iteration(gold, dev="cpu"):
    """tests/golden/mapper_ba.npz's first BA iteration as tensors: oracle-style parameters P (the table regenerated from
    its seed: the fixture's mapper ran with grid_lr = 0), rays, z_vals, dists, camera parameters, their gradients, and
    the rays per visit_list entry (runs of equal origins: an entry's rays all start at its t)."""
    from oracle import neus_oracle as NO
    T = lambda k: torch.from_numpy(gold[k])
    bound = T("first_net.bound")
    P = NO.make_params(int(gold["seed_net"]), grid_init=0.3,
                       bound=tuple(tuple(float(x) for x in r) for r in bound))
    P.update(sdf_w=T("first_net.sdf_network.sdf_layer.weight"), sdf_b=T("first_net.sdf_network.sdf_layer.bias"),
             color_B=T("first_net.color_network._B"), mlp=T("first_net.color_network.network.params"),
             variance=T("first_net.variance_network.variance"), rt_bound=T("first_net.realtime_bound"), bound=bound)
    o = T("first_rays_o")
    change = torch.ones(o.shape[0], dtype=torch.bool)
    change[1:] = (o[1:] != o[:-1]).any(1)
    starts = torch.nonzero(change).reshape(-1).tolist() + [o.shape[0]]
    counts = [b - a for a, b in zip(starts[:-1], starts[1:])]
    return dict(P=P, rays_o=o, rays_d=T("first_rays_d"), color=T("first_color"), depth=T("first_depth"),
                z=T("first_z"), dists=T("first_dists"), cam=T("first_cam_param"), cam_grad=T("first_cam_grad"),
                counts=counts)


def camera_gradients(F, ray_grad_fn):
    """dL/dq for the fixture's first iteration: rays rebuilt from the camera parameters (rays_d = dirs R^T, rays_o = t,
    dirs = the recorded rays_d R), then `ray_grad_fn(rays_o, rays_d) -> (dL/d rays_o, dL/d rays_d)` chained back
    through quad2rotation by autograd"""
    from go_slam_amd.neus.pose import quaternion_to_rt
    q = F["cam"].double().clone().requires_grad_(True)
    c2w = quaternion_to_rt(q)
    R, t = c2w[:, :3, :3], c2w[:, :3, 3]
    e = torch.repeat_interleave(torch.arange(len(F["counts"])), torch.tensor(F["counts"]))
    dirs = (F["rays_d"].double()[:, :, None] * R.detach()[e]).sum(1)           # d R  (R orthonormal: R^T R = I)
    rays_d = (dirs[:, None, :] * R[e]).sum(-1)
    rays_o = t[e]
    go, gd = ray_grad_fn(rays_o.detach().float(), rays_d.detach().float(), dirs.float())
    torch.autograd.backward([rays_o, rays_d], [go.double(), gd.double()])
    return q.grad, dirs.float(), e
