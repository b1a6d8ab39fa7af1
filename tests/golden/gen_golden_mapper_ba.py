#!/usr/bin/env python
"""Generate tests/golden/mapper_ba.npz by RUNNING THE REFERENCE'S OWN Mapper with `mapping.BA: True`.

    python tests/golden/gen_golden_mapper_ba.py         # needs the reference tree (as gen_golden.py does)

Reuses gen_golden.py's stand-ins by import: the twice-differentiable tinycudann stand-in (`differentiable_tcnn`, whose
encoding is differentiable in its input, so the reference's rays reach the camera parameters), the reference's own
DepthVideo, InstantNeuS, Renderer and Mapper on the CPU.  mathutils is not installed: it is stubbed by `Matrix` with a
restated `to_quaternion` (the unit quaternion of the column-normalised rotation, Shepperd's branches).  The reference's
`quad2rotation` calls `.to(quad.get_device())`, which is -1 for a CPU tensor; `Tensor.get_device` is made to return the
CPU device while the Mapper runs.

The mapper runs with grid_lr = 0 (the table is regenerated from its seed by the tests) and pixels = 240.
Schedule (filtered_id): 5 (first call), 14 (last_visit 5: no BA), 30 (last_visit 14 >= 10: BA on), 30 again with
keyframe 29's priority raised so that it is both a "recent" and a "priority" entry of visit_list (two camera parameters
for one keyframe).  NumPy and torch are re-seeded before every call.  Recorded: every visit ray batch of the BA calls,
the camera parameters' gradients at the first BA iteration with the network parameters, z_vals and dists of that moment,
the camera parameters after each BA call, the camera group's hyperparameters and visit lists."""
import importlib
import importlib.util
import math
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
SCHEDULE = (5, 14, 30, 30)
SEED_NET = 223
BA_CAM_LR = 2.5e-3


def load_gen():
    spec = importlib.util.spec_from_file_location("gen_golden", os.path.join(HERE, "gen_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def ba_cfg(gen):
    cfg = gen.mapper_cfg()
    # grid_lr = 0: the 12.6 M-entry hash table stays at its seeded values (net_params), so the fixture need not store it;
    # the dense parameters train at net_lr and are recorded
    cfg["mapping"].update(BA=True, BA_cam_lr=BA_CAM_LR, pixels=240, grid_lr=0.0)
    return cfg


def net_cfg():
    return {"sdf_network": {"d_in": 3, "d_out": 32},
            "color_network": {"d_in": 3, "d_feat": 31, "d_hidden": 64, "n_layers": 2},
            "variance_network": {"init_val": 0.2, "scale_factor": 10.0}, "sdf_smooth_std": 0.005,
            "sdf_sparse_factor": 5, "sdf_truncation": 0.16, "sdf_random_weight": 0.04}


def net_params(bound):
    from oracle import neus_oracle as NO
    return NO.make_params(SEED_NET, grid_init=0.3, bound=tuple(tuple(float(x) for x in r) for r in bound))


def prepare_call(video, k, fid):
    """the state every implementation sets before call k (seeds, filtered_id, keyframe 29's priority on the last call)"""
    video.filtered_id[0] = fid
    if k == len(SCHEDULE) - 1:
        video.update_priority[29] = 100.0
    np.random.seed(3000 + k)
    torch.manual_seed(4000 + k)


def install_mathutils():
    mu = types.ModuleType("mathutils")

    class Matrix:
        def __init__(self, rows):
            self.m = np.asarray(rows, dtype=np.float64)

        def to_quaternion(self):
            R = self.m / np.linalg.norm(self.m, axis=0, keepdims=True)
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
            return np.asarray(q) / np.linalg.norm(q)
    mu.Matrix = Matrix
    sys.modules["mathutils"] = mu


def main():
    gen = load_gen()
    gen.install_stubs()
    install_mathutils()
    keep = gen.differentiable_tcnn()
    sys.modules["refsrc.geom"].projective_ops = importlib.import_module("refsrc.geom.projective_ops")
    gen.droid_modules()
    dv = importlib.import_module("refsrc.depth_video")
    neus = importlib.reload(importlib.import_module("refsrc.InstantNeuS"))
    render = importlib.import_module("refsrc.render")
    mp = importlib.import_module("refsrc.mapping")
    torch.autograd.set_detect_anomaly(False)                                # mapping.py switches it on at import
    cfg = ba_cfg(gen)
    video = dv.DepthVideo(cfg, types.SimpleNamespace(device="cpu"))
    gen.fill_mapping_video(video)
    bound = video.bound[0].clone()
    P = net_params(bound)
    torch.manual_seed(5)
    net = neus.InstantNeuS(net_cfg(), bound.tolist(), device="cpu")
    with torch.no_grad():
        net.sdf_network.encoding.encoding.params.copy_(P["grid"])
        net.sdf_network.sdf_layer.weight.copy_(P["sdf_w"])
        net.sdf_network.sdf_layer.bias.copy_(P["sdf_b"])
        net.color_network._B.copy_(P["color_B"])
        net.color_network.network.params.copy_(P["mlp"])
    renderer = render.Renderer({"rendering": {"lindisp": False, "perturb": 1.0, "N_samples": 24, "N_surface": 48}},
                               None, types.SimpleNamespace(H=32, W=48, fx=40.0, fy=41.0, cx=24.0, cy=16.0))
    slam = types.SimpleNamespace(verbose=False, bound=bound, video=video, mapping_net=net, renderer=renderer,
                                 reload_map=torch.zeros(1).int(), output=tempfile.mkdtemp(), H=32, W=48, fx=40.0,
                                 fy=41.0, cx=24.0, cy=16.0)
    mapper = mp.Mapper(cfg, types.SimpleNamespace(device="cpu"), slam)
    out, batches, first = {}, [], {}
    real_opt, real_fwd = mapper.optimize_map, net.forward
    opt = mapper.optimizer
    real_step = opt.step

    def optimize_map(rays_o, rays_d, rays_color, rays_depth, optimizer, num_joint_iters):
        ba = len(optimizer.param_groups) > 2 and rays_o.requires_grad
        if ba:
            batches.append([t.detach().clone() for t in (rays_o, rays_d, rays_color, rays_depth)])
            if not first:
                first["state"] = {k: v.detach().clone() for k, v in net.state_dict().items()}
                first["rays"] = batches[-1]
        return real_opt(rays_o, rays_d, rays_color, rays_depth, optimizer, num_joint_iters)

    def forward(rays_o, rays_d, z_vals, dists, render_params=None):
        if "state" in first and "z" not in first:
            first["z"], first["dists"] = z_vals.detach().clone(), dists.detach().clone()
        return real_fwd(rays_o, rays_d, z_vals, dists, render_params)

    def step(*a, **kw):
        g = opt.param_groups[-1]
        if len(opt.param_groups) > 2 and "cam_grad" not in first and g["params"][0].grad is not None:
            first["cam_grad"] = torch.stack([p.grad.detach().clone() for p in g["params"]])
            first["cam_param"] = torch.stack([p.detach().clone() for p in g["params"]])
        return real_step(*a, **kw)
    mapper.optimize_map, net.forward, opt.step = optimize_map, forward, step
    real_get_device = torch.Tensor.get_device
    torch.Tensor.get_device = lambda self: self.device if self.device.type == "cpu" else real_get_device(self)
    try:
        for k, fid in enumerate(SCHEDULE):
            prepare_call(video, k, fid)
            n0 = len(batches)
            mapper()
            pg = opt.param_groups
            out[f"call{k}_groups"] = np.array(len(pg))
            out[f"call{k}_batches"] = np.array([n0, len(batches)])
            if len(pg) > 2:
                out[f"call{k}_cam"] = torch.stack([p.detach().clone() for p in pg[-1]["params"]])
                out[f"call{k}_hyper"] = torch.tensor([pg[-1]["lr"], pg[-1]["weight_decay"], pg[-1]["betas"][0],
                                                      pg[-1]["betas"][1], pg[-1]["eps"]], dtype=torch.float64)
    finally:
        torch.Tensor.get_device = real_get_device
        tc = sys.modules["tinycudann"]
        tc.Encoding, tc.Network = keep
    for i, b in enumerate(batches):
        for name, t in zip(("rays_o", "rays_d", "color", "depth"), b):
            out[f"batch{i}_{name}"] = t
    out["n_batches"] = np.array(len(batches))
    grid_key = "sdf_network.encoding.encoding.params"
    assert torch.equal(first["state"][grid_key], P["grid"].float()), "grid_lr = 0 must leave the table untouched"
    for k, v in first["state"].items():
        if k != grid_key:
            out["first_net." + k] = v
    for name in ("z", "dists", "cam_grad", "cam_param"):
        out["first_" + name] = first[name]
    for name, t in zip(("rays_o", "rays_d", "color", "depth"), first["rays"]):
        out["first_" + name] = t
    out["realtime_bound"] = net.realtime_bound.detach().clone()
    out["ba_cam_lr"] = np.array(BA_CAM_LR)
    out["seed_net"] = np.array(SEED_NET)
    np.savez_compressed(os.path.join(HERE, "mapper_ba.npz"),
                        **{k: (v.numpy() if torch.is_tensor(v) else v) for k, v in out.items()})
    print("wrote mapper_ba.npz:", len(batches), "BA batches,", {k: v.shape for k, v in out.items() if "call" in k})


if __name__ == "__main__":
    main()
