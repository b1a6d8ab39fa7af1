"""mapping.BA on the GPU: ray gradients of the HIP NeuS backward (gs_neus_backward_raygrad), the per-pose reduction
(gs_pose_grad_reduce), the fused step's ray-gradient form and Mapper.__call__ with camera refinement.

Referee: tests/pose_grad_restatement.py (oracle/neus_autograd's differentiable forward with differentiable sample points,
grid input derivatives of first and second order) under torch.autograd on the CPU.  Bounds are relative norms, as the
parameter-gradient tests of test_neus_gpu.py use (5e-3)."""
import importlib.util
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def N(built_lib):
    import go_slam_amd.neus as neus
    return neus


def _restatement():
    spec = importlib.util.spec_from_file_location("pose_grad_restatement", os.path.join(HERE, "pose_grad_restatement.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp(min=1e-12))


def _problem(seed, n=48, rt=((-2.2, 2.3), (-2.4, 2.1), (-2.0, 2.2)), zero_frac=0.2):
    from oracle import neus_oracle as O
    P = O.make_params(seed, grid_init=0.3, bound=((-2.5, 2.5), (-2.5, 2.5), (-2.5, 2.5)))
    P["rt_bound"] = torch.tensor(rt)
    P["variance"] = torch.tensor(0.2)
    g = torch.Generator().manual_seed(seed + 1)
    o = torch.rand(n, 3, generator=g) * 4 - 2
    d = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=1) * (0.8 + 0.4 * torch.rand(n, 1, generator=g))
    gt = torch.rand(n, generator=g) * 3.5 + 0.5
    gt[torch.rand(n, generator=g) < zero_frac] = 0                    # depth-less rays
    z, dist = O.render_sample(o, d, gt, P["bound"], 24, 48, torch.rand(24, generator=g))
    col = torch.rand(n, 3, generator=g)
    return P, o, d, gt, z, dist, col


def _model(N, P, dev):
    m = N.InstantNeuS({}, P["bound"].tolist()).to(dev)
    with torch.no_grad():
        m.sdf_network.encoding.encoding.params.copy_(P["grid"])
        m.sdf_network.sdf_layer.weight.copy_(P["sdf_w"])
        m.sdf_network.sdf_layer.bias.copy_(P["sdf_b"])
        m.color_network._B.copy_(P["color_B"])
        m.color_network.network.params.copy_(P["mlp"])
        m.variance_network.variance.fill_(float(P["variance"]))
    m.update_bound(P["rt_bound"])
    return m


def _losses(n, seed):
    from oracle import neus_autograd as NA
    g = torch.Generator().manual_seed(seed)
    wc, wd, wn = torch.randn(n, 3, generator=g), torch.randn(n, 1, generator=g), torch.randn(n, 3, generator=g)
    ws = torch.randn(n, 72, generator=g)
    on = lambda w, ref: w.to(ref.device)
    return {
        "color": lambda out: (out["color"] * on(wc, out["color"])).sum(),
        "depth": lambda out: (out["depth"] * on(wd, out["depth"])).sum(),
        "sdf": lambda out: (out["sdf"] * on(ws, out["sdf"])).sum(),
        "eikonal": lambda out: out["gradient_error"].sum() * 100.0,
        "normal": lambda out: (out["normal"] * on(wn, out["normal"])).sum(),
        "full": None,       # NA.mapping_loss, bound below with the batch's colours and depths
    }, NA


def _hip_ray_grads(N, P, o, d, z, dist, loss_fn, dev, grad_params=True):
    model = _model(N, P, dev)
    if not grad_params:
        for p in model.parameters():
            p.requires_grad_(False)
    ro = o.to(dev).clone().requires_grad_(True)
    rd = d.to(dev).clone().requires_grad_(True)
    out = model(ro, rd, z.to(dev), dist.to(dev))
    loss_fn(out).backward()
    return ro.grad.cpu(), rd.grad.cpu(), model


@pytest.mark.parametrize("term", ["color", "depth", "sdf", "eikonal", "normal", "full"])
@pytest.mark.parametrize("case", ["mixed", "forced_first_100"])
def test_ray_gradients_match_restatement(N, dev, term, case):
    """dL/d rays_o, dL/d rays_d of InstantNeuS.forward (HIP backward + gs_neus_backward_raygrad) vs autograd on the
    restatement, per loss term isolated and for the mapper's full loss.  `mixed`: samples outside the realtime bound
    and rays without depth; `forced_first_100`: a realtime bound that contains no sample (mask[:100] = True)."""
    R = _restatement()
    rt = ((-2.2, 2.3), (-2.4, 2.1), (-2.0, 2.2)) if case == "mixed" else ((9.0, 9.5), (9.0, 9.5), (9.0, 9.5))
    P, o, d, gt, z, dist, col = _problem(31, rt=rt)
    losses, NA = _losses(o.shape[0], 32)
    fn = losses[term] or (lambda out: NA.mapping_loss(out, col.to(out["color"].device), gt.to(out["color"].device)))
    ref_o, ref_d = R.ray_gradients(o, d, z, dist, P, fn)
    got_o, got_d, _ = _hip_ray_grads(N, P, o, d, z, dist, fn, dev)
    rep = {"rays_o": _rel(got_o, ref_o), "rays_d": _rel(got_d, ref_d)}
    assert float(ref_o.norm()) > 0 and float(ref_d.norm()) > 0
    assert all(v < 5e-3 for v in rep.values()), rep


def test_parameter_gradients_do_not_change_when_ray_gradients_are_requested(N, dev):
    """the dense parameters' gradients are bitwise those of the backward without ray gradients (the ray pass reads the
    backward's inputs and writes only its own buffers).  The table gradient and d variance cannot be compared bitwise:
    even two runs WITHOUT ray gradients differ there -- the dense levels' table gradient is summed by fp16 packed atomics
    and d inv_s by one float atomic per workgroup, in whatever order the workgroups finish (test_neus_gpu.py's fused-step
    test documents the same).  They are held to that noise."""
    P, o, d, gt, z, dist, col = _problem(41)
    from oracle import neus_autograd as NA
    fn = lambda out: NA.mapping_loss(out, col.to(dev), gt.to(dev))
    grads = []
    for want in (False, True):
        model = _model(N, P, dev)
        ro, rd = o.to(dev).requires_grad_(want), d.to(dev).requires_grad_(want)
        fn(model(ro, rd, z.to(dev), dist.to(dev))).backward()
        grads.append({k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None})
        assert (ro.grad is not None) == want
    a, b = grads
    assert a.keys() == b.keys()
    for k in a:
        if k.endswith("encoding.params"):
            assert _rel(b[k].cpu(), a[k].cpu()) < 1e-3, k
        elif k.endswith("variance"):        # (d inv_s: one float atomic per workgroup)
            torch.testing.assert_close(b[k], a[k], rtol=1e-5, atol=0)
        else:
            assert torch.equal(a[k], b[k]), k


def test_ray_and_pose_gradients_are_bitwise_reproducible(N, dev):
    from go_slam_amd.neus.pose import pose_gradients
    P, o, d, gt, z, dist, col = _problem(51, n=300)
    from oracle import neus_autograd as NA
    fn = lambda out: NA.mapping_loss(out, col.to(dev), gt.to(dev))
    runs = []
    seg = torch.tensor([0, 100, 101, 300], dtype=torch.int32, device=dev)
    for _ in range(2):
        go, gd, _ = _hip_ray_grads(N, P, o, d, z, dist, fn, dev)
        rg = torch.cat([go, gd], 1).to(dev).contiguous()
        dR, dt = pose_gradients(rg, d.to(dev).contiguous(), seg)
        runs.append((go, gd, dR.cpu(), dt.cpu()))
    for x, y in zip(*runs):
        assert torch.equal(x, y)


@pytest.mark.parametrize("counts", [[37], [1, 0, 130, 64, 65, 7, 3, 200, 1, 17, 19, 23, 29, 31, 2, 5, 8, 13, 21, 34, 55, 89],
                                    [4096 + 33]])
def test_pose_reduction_matches_fp64_sum_at_ragged_segments(N, dev, counts):
    from go_slam_amd.neus.pose import pose_gradients
    R = _restatement()
    n = sum(counts)
    g = torch.Generator().manual_seed(n)
    rg = torch.randn(n, 6, generator=g)
    dirs = torch.randn(n, 3, generator=g)
    seg = torch.tensor([0] + list(np.cumsum(counts)), dtype=torch.int32, device=dev)
    dR, dt = pose_gradients(rg.to(dev), dirs.to(dev), seg)
    rR, rt = R.pose_gradients_fp64(rg, dirs, counts)
    torch.testing.assert_close(dR.cpu().double(), rR, rtol=0, atol=1e-5 * max(1.0, n ** 0.5))
    torch.testing.assert_close(dt.cpu().double(), rt, rtol=0, atol=1e-5 * max(1.0, n ** 0.5))


def test_fused_step_ray_gradients_equal_the_autograd_step(N, dev):
    """MapTrainer.step_ray_grad on the fused step (loss kernel -> HIP backward incl. the ray pass) vs the autograd
    step (InstantNeuS.forward differentiable in the rays, torch loss); and both trainers take the same network step"""
    from go_slam_amd.neus.mapper import MapTrainer
    from oracle import neus_oracle as O
    P, o, d, gt, z, dist, col = _problem(61, n=512)
    pr = torch.rand(24, generator=torch.Generator().manual_seed(62))
    res = []
    for fused in (False, True):
        model = _model(N, P, dev)
        t = MapTrainer(model, N.Renderer(N_samples=24, N_surface=48), fused=fused)
        loss, d_rays = t.step_ray_grad(o.to(dev), d.to(dev), col.to(dev), gt.to(dev), pr.to(dev))
        res.append((float(loss), d_rays.cpu()))
    (la, ga), (lf, gf) = res
    assert abs(la - lf) <= 2e-4 * abs(la) + 1e-5
    rep = {"rays_o": _rel(gf[:, :3], ga[:, :3]), "rays_d": _rel(gf[:, 3:], ga[:, 3:])}
    # pose gradients: the fused step's rays -> gs_pose_grad_reduce vs autograd's own scatter of the autograd step's rays
    # through rays_d = dirs R^T, rays_o = t (22 ragged entries)
    from go_slam_amd.neus.pose import pose_gradients
    counts = [23 * (k % 3) + 1 for k in range(21)]
    counts.append(512 - sum(counts))
    seg = torch.tensor([0] + list(np.cumsum(counts)), dtype=torch.int32, device=dev)
    dirs = d.contiguous()
    dR, dt = pose_gradients(gf.to(dev).contiguous(), dirs.to(dev), seg)
    Rs = torch.eye(3).repeat(22, 1, 1).requires_grad_(True)
    ts = torch.zeros(22, 3, requires_grad=True)
    e = torch.repeat_interleave(torch.arange(22), torch.tensor(counts))
    torch.autograd.backward([(dirs[:, None, :] * Rs[e]).sum(-1), ts[e]], [ga[:, 3:], ga[:, :3]])
    rep["dR"], rep["dt"] = _rel(dR.cpu(), Rs.grad), _rel(dt.cpu(), ts.grad)
    print("fused step vs autograd step:", rep)
    assert all(v < 1e-3 for v in rep.values()), rep     # measured: rays 0 (bitwise), dR / dt 1.3e-7


def _gen():
    spec = importlib.util.spec_from_file_location("gen_golden", os.path.join(HERE, "golden", "gen_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def _gen_ba():
    spec = importlib.util.spec_from_file_location("gen_golden_mapper_ba",
                                                  os.path.join(HERE, "golden", "gen_golden_mapper_ba.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_pose_chain_reproduces_the_reference_mappers_first_iteration_gradients(N, dev):
    """The product's chain on the fixture's first BA iteration (tests/golden/mapper_ba.npz, the reference's own Mapper):
    HIP ray gradients of InstantNeuS.forward -> gs_pose_grad_reduce -> quaternion_to_rt backward gives the reference's
    camera gradients.  Catches a transposed R, a wrong segment order or o/d half, a wrong quaternion convention."""
    R = _restatement()
    from go_slam_amd.neus.pose import pose_gradients
    from oracle import neus_autograd as NA
    gold = np.load(os.path.join(HERE, "golden", "mapper_ba.npz"))
    F = R.fixture_first_iteration(gold)
    model = _model(N, F["P"], dev)
    seg = torch.tensor([0] + list(np.cumsum(F["counts"])), dtype=torch.int32, device=dev)
    got = {}

    def hip(o, d, dirs):
        ro, rd = o.to(dev).requires_grad_(True), d.to(dev).requires_grad_(True)
        out = model(ro, rd, F["z"].to(dev), F["dists"].to(dev))
        NA.mapping_loss(out, F["color"].to(dev), F["depth"].to(dev)).backward()
        rg = torch.cat([ro.grad, rd.grad], 1).contiguous()
        got["pose"] = pose_gradients(rg, dirs.to(dev).contiguous(), seg)
        return ro.grad.cpu(), rd.grad.cpu()
    g, dirs, e = R.camera_gradients(F, hip)
    ref = F["cam_grad"].double()
    rel = _rel(g, ref)
    print("first-iteration camera gradients vs the reference Mapper: rel", rel)
    assert rel < 5e-3, rel              # measured 8.6e-5 (the restatement's own distance to the fixture: 8.6e-5)
    # the chain again with the HIP pose reduction's dL/dR, dL/dt in place of autograd's scatter
    from go_slam_amd.neus.pose import quaternion_to_rt
    q = F["cam"].double().clone().requires_grad_(True)
    c2w = quaternion_to_rt(q)
    dR, dt = got["pose"]
    torch.autograd.backward([c2w[:, :3, :3], c2w[:, :3, 3]], [dR.cpu().double(), dt.cpu().double()])
    rel2 = _rel(q.grad, ref)
    print("... through gs_pose_grad_reduce: rel", rel2)
    assert rel2 < 5e-3, rel2            # measured 8.6e-5


class _CpuDraws:
    """torch.randint / torch.rand on the CPU generator, moved to the device: the reference's Mapper drew its pixels and
    perturbations on the CPU, so a CUDA Mapper under this patch draws the same ones (test harness only)"""

    def __enter__(self):
        self.ri, self.r = torch.randint, torch.rand
        ri, r = self.ri, self.r

        def randint(*a, device=None, out=None, **kw):
            t = ri(*a, **kw)
            if out is not None:
                return out.copy_(t)
            return t.to(device) if device is not None else t

        def rand(*a, device=None, **kw):
            t = r(*a, **kw)
            return t.to(device) if device is not None else t
        torch.randint, torch.rand = randint, rand
        return self

    def __exit__(self, *exc):
        torch.randint, torch.rand = self.ri, self.r
        return False


def test_mapper_call_with_ba_matches_the_reference_mapper(N, dev):
    """Mapper.__call__ with mapping.BA on CUDA vs the reference's own Mapper (tests/golden/mapper_ba.npz, same video,
    network, schedule and seeds): no camera group before last_visit >= 10; the group's lr (BA_cam_lr = 2.5e-3 from the
    config), weight decay, betas, eps; one parameter per visit_list entry incl. keyframe 29 twice on the last call; a new
    group on every call; the same BA ray batches; the same poses after each call; the video's poses untouched."""
    from go_slam_amd.depth_video import DepthVideo
    from go_slam_amd.neus.mapping import Mapper
    gen, gba = _gen(), _gen_ba()
    gold = np.load(os.path.join(HERE, "golden", "mapper_ba.npz"))
    cfg = gba.ba_cfg(gen)
    cfg["mapping"]["device"] = "cuda:0"
    video = DepthVideo.from_config(cfg, types.SimpleNamespace(device="cpu"))
    gen.fill_mapping_video(video)
    poses_before = video.poses_filtered.clone()
    bound = video.bound[0].clone()
    P = gba.net_params(bound)
    P["rt_bound"], P["variance"] = bound, torch.tensor(0.2)
    net = _model(N, P, dev)
    slam = types.SimpleNamespace(verbose=False, bound=bound, video=video, mapping_net=net,
                                 renderer=N.Renderer(N_samples=24, N_surface=48), reload_map=torch.zeros(1).int(),
                                 H=32, W=48, fx=40.0, fy=41.0, cx=24.0, cy=16.0)
    mapper = Mapper(cfg, types.SimpleNamespace(device="cuda:0"), slam)
    batches, real = [], mapper.trainer.step_ray_grad

    def rec(rays_o, rays_d, color, depth, *a, **kw):
        batches.append([t.detach().cpu().clone() for t in (rays_o, rays_d, color, depth)])
        return real(rays_o, rays_d, color, depth, *a, **kw)
    mapper.trainer.step_ray_grad = rec
    lr = float(gold["ba_cam_lr"])
    groups, report = [], {}
    with _CpuDraws():
        for k, fid in enumerate(gba.SCHEDULE):
            gba.prepare_call(video, k, fid)
            mapper()
            pg = mapper.optimizer.param_groups
            assert len(pg) == int(gold[f"call{k}_groups"]), k
            assert len(batches) == int(gold[f"call{k}_batches"][1]), k
            if len(pg) == 2:
                assert mapper.cam_params is None
                continue
            cam = pg[2]
            hyper = [cam["lr"], cam["weight_decay"], cam["betas"][0], cam["betas"][1], cam["eps"]]
            assert np.allclose(hyper, gold[f"call{k}_hyper"], rtol=1e-12, atol=0), hyper
            assert len({id(p) for p in cam["params"]}) == len(cam["params"]) == gold[f"call{k}_cam"].shape[0]
            assert all(a is b for a, b in zip(cam["params"], mapper.cam_params))
            groups.append(cam)
            got = torch.stack([p.detach().cpu() for p in cam["params"]])
            ref = torch.from_numpy(gold[f"call{k}_cam"])
            # after `iters` = 2 AdamW steps each component has moved by ~lr per step; a component whose gradient changes
            # sign between the two implementations (the networks differ by fp16-table rounding) can end 2 lr x steps
            # apart.  Bound: 4 lr per component; and most components within lr / 10
            d = (got - ref).abs()
            report[f"call{k}"] = (float(d.max()), float((d <= lr / 10).float().mean()))
            assert float(d.max()) <= 4 * lr, report                      # measured 0.23 lr (call 2), 0.015 lr
            assert float((d <= lr / 10).float().mean()) >= 0.9, report  # measured 0.97, 1.0
    print("post-call poses vs the reference (max |dq|, fraction within lr/10):", report)
    assert len(groups) == 2 and groups[0] is not groups[1]
    assert not any(a is b for a in groups[0]["params"] for b in groups[1]["params"])
    # the pixels are the reference's; the rays of a call's first iteration come from the same unrefined poses, later
    # ones from poses one AdamW step (<= ~lr per component) apart
    assert len(batches) == int(gold["n_batches"])
    for i, b in enumerate(batches):
        ro, rd, col, dep = (torch.from_numpy(gold[f"batch{i}_{n}"]) for n in ("rays_o", "rays_d", "color", "depth"))
        assert torch.equal(b[2], col) and torch.equal(b[3], dep.reshape(-1)), i
        tol = 1e-5 if i % 2 == 0 else 8 * lr * (1.0 + float(rd.abs().max()))
        torch.testing.assert_close(b[0], ro, rtol=0, atol=tol, msg=lambda m: f"batch {i}: {m}")
        torch.testing.assert_close(b[1], rd, rtol=0, atol=tol, msg=lambda m: f"batch {i}: {m}")
    assert torch.equal(video.poses_filtered, poses_before)
