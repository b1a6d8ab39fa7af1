"""mapping.BA host side: the pose helpers that replace mathutils (reference src/nerf_func.py:44-112) and the ray-gradient
restatement the GPU tests use as their referee (tests/pose_grad_restatement.py)."""
import importlib.util
import math
import os

import numpy as np
import torch

from go_slam_amd.lietorch_shim import SE3
from go_slam_amd.neus.pose import quad2rotation, quaternion_to_rt, rt_to_quaternion

HERE = os.path.dirname(os.path.abspath(__file__))


def _restatement():
    spec = importlib.util.spec_from_file_location("pose_grad_restatement", os.path.join(HERE, "pose_grad_restatement.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _poses(n, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return SE3.exp(scale * torch.randn(n, 6, generator=g, dtype=torch.float64)).matrix()


def test_quaternion_round_trip_and_unit_norm():
    for T in _poses(64, 1, scale=1.5):
        q = rt_to_quaternion(T.float())
        assert q.dtype == torch.float32 and q.shape == (7,)
        assert abs(float(q[:4].double().norm()) - 1.0) < 1e-6
        back = quaternion_to_rt(q.double())
        torch.testing.assert_close(back, T, rtol=0, atol=2e-6)


def test_quaternion_near_180_degree_rotations():
    """the trace of R approaches -1: Shepperd's branches on the largest diagonal entry keep the conversion exact"""
    for axis in ([1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0], [1.0, 1.0, 0], [0.3, -0.5, 0.8]):
        a = torch.tensor(axis, dtype=torch.float64)
        a = a / a.norm()
        for ang in (math.pi, math.pi - 1e-4, math.pi - 1e-2):
            T = SE3.exp(torch.cat([torch.tensor([0.5, -1.0, 2.0], dtype=torch.float64), a * ang])[None]).matrix()[0]
            q = rt_to_quaternion(T)
            assert abs(float(q[:4].double().norm()) - 1.0) < 1e-6
            torch.testing.assert_close(quaternion_to_rt(q.double()), T, rtol=0, atol=2e-6)


def test_quad2rotation_matches_the_reference_formula_in_fp64_and_ignores_the_norm():
    R = _restatement()
    g = torch.Generator().manual_seed(5)
    q = torch.randn(50, 4, generator=g, dtype=torch.float64) * 3.0          # off the unit sphere, as AdamW leaves it
    torch.testing.assert_close(quad2rotation(q), R.quad2rotation_fp64(q), rtol=0, atol=1e-14)
    torch.testing.assert_close(quad2rotation(q), quad2rotation(q / q.norm(dim=1, keepdim=True)), rtol=0, atol=1e-13)
    t = torch.randn(50, 3, generator=g, dtype=torch.float64)
    Rt = quaternion_to_rt(torch.cat([q, t], 1))
    assert Rt.shape == (50, 4, 4) and torch.equal(Rt[:, :3, 3], t)
    assert torch.equal(Rt[:, 3], torch.tensor([0.0, 0, 0, 1], dtype=torch.float64).expand(50, 4))


def test_restatement_forward_equals_the_oracle_and_is_differentiable_in_the_rays():
    """the referee's forward is oracle/neus_autograd.neus_forward_diff value for value (only the derivatives in the
    sample points are added), and every output that depends on the points reaches both rays_o and rays_d"""
    Rmod = _restatement()
    from oracle import neus_autograd as NA, neus_oracle as NO
    P = NO.make_params(7, grid_init=0.3, bound=((-2.5, 2.5), (-2.5, 2.5), (-2.5, 2.5)))
    P["rt_bound"] = torch.tensor([[-2.2, 2.3], [-2.4, 2.1], [-2.0, 2.2]])
    P["variance"] = torch.tensor(0.2)
    g = torch.Generator().manual_seed(8)
    n = 16
    o = torch.rand(n, 3, generator=g) * 4 - 2
    d = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=1)
    gt = torch.rand(n, generator=g) * 3 + 0.5
    z, dist = NO.render_sample(o, d, gt, P["bound"], 24, 48, torch.rand(24, generator=g))
    ref = NA.neus_forward_diff(o, d, z, dist, P)
    got = Rmod.neus_forward_rays_diff(o, d, z, dist, P)
    for k in ("color", "depth", "depth_variance", "normal", "weight_sum", "sdf", "z_vals", "gradient_error"):
        torch.testing.assert_close(got[k], ref[k], rtol=0, atol=0, msg=k)
    for k in ("color", "depth", "normal", "gradient_error"):
        go, gd = Rmod.ray_gradients(o, d, z, dist, P, lambda out: out[k].sum())
        assert float(go.norm()) > 0 and float(gd.norm()) > 0, k
        assert torch.isfinite(go).all() and torch.isfinite(gd).all(), k


def test_pose_gradient_chain_rule_of_the_fp64_reduction():
    """dL/dR = sum dL/d rays_d^T dirs, dL/dt = sum dL/d rays_o: the reduction's definition checked by autograd through
    rays_d = dirs @ R^T, rays_o = t with ragged segments"""
    Rmod = _restatement()
    counts = [1, 5, 0, 9]
    g = torch.Generator().manual_seed(3)
    dirs = torch.randn(sum(counts), 3, generator=g, dtype=torch.float64)
    Rs = torch.randn(4, 3, 3, generator=g, dtype=torch.float64, requires_grad=True)
    ts = torch.randn(4, 3, generator=g, dtype=torch.float64, requires_grad=True)
    e = torch.repeat_interleave(torch.arange(4), torch.tensor(counts))
    rd = (dirs[:, None, :] * Rs[e]).sum(-1)
    ro = ts[e]
    w = torch.randn(sum(counts), 6, generator=g, dtype=torch.float64)
    ((ro * w[:, :3]).sum() + (rd * w[:, 3:]).sum()).backward()
    dR, dt = Rmod.pose_gradients_fp64(w, dirs, counts)
    torch.testing.assert_close(dR, Rs.grad)
    torch.testing.assert_close(dt, ts.grad)


def test_restatement_reproduces_the_reference_mappers_first_iteration_camera_gradients():
    """tests/golden/mapper_ba.npz: the reference's own Mapper (BA on, CPU, tinycudann stand-in differentiable in its
    input) recorded its camera parameters' gradients at the first BA iteration, with the network parameters, z_vals and
    dists of that moment.  The restatement, chained through quad2rotation, gives the same gradients.  Bound: relative
    norm 2e-3 -- the reference rounds the gradient reaching the encoding output to fp16 (tcnn; the restatement does not);
    measured 8.6e-5."""
    Rmod = _restatement()
    from oracle import neus_autograd as NA
    gold = np.load(os.path.join(HERE, "golden", "mapper_ba.npz"))
    F = Rmod.fixture_first_iteration(gold)
    loss = lambda out: NA.mapping_loss(out, F["color"], F["depth"])
    g, _, _ = Rmod.camera_gradients(F, lambda o, d, dirs: Rmod.ray_gradients(o, d, F["z"], F["dists"], F["P"], loss))
    ref = F["cam_grad"].double()
    rel = float((g - ref).norm() / ref.norm())
    assert len(F["counts"]) == ref.shape[0] and rel < 2e-3, rel
