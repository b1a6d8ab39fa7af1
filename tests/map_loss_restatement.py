"""The mapper's loss in float64 on the CPU: the referee of gs_mapping_loss (go_slam_amd/csrc/map_loss.hip) and of the
unfused torch path of go_slam_amd/neus/distributed.mapping_loss_sharded.

Written from the reference's formulation (src/mapping.py:96-132 with InstantNeuS.compute_sdf_error,
src/InstantNeuS.py:372-400): the rays with a depth measurement are GATHERED, every term is a mean over them, and the
gradients w.r.t. the renderer's outputs come from autograd on the float64 loss.  The only departure is the one the sharded
mapper needs: the means over valid rays divide by a count that is passed in (`count`, the global number of valid rays)
instead of the local one; with one rank they are the same number.

`CASES` maps a name to the inputs of one launch.  Every tensor value is an fp32 number on the dyadic grid k / 1024 with
|value| < 8, so gt - z, pred - (gt - z), color - rays_color and depth - gt are exact in fp32, and every sign and mask is the
same in fp32 and fp64.  The truncation 0.16 is off the grid (163 / 1024 < 0.16 < 164 / 1024: no sample within 8e-4 of a mask
boundary); the `boundary` case uses 0.125 = 128 / 1024 and puts samples exactly on gt - trunc and gt + trunc.

The error bounds of both code paths (in units of u = 2^-24) are derived in tests/test_map_loss_numerics_gpu.py; the numbers
live here because tests/test_map_loss_cpu.py measures wrong variants of this restatement against the same bounds."""
import numpy as np
import torch

U = 2.0 ** -24
Q = 1024.0                       # the grid: every input is an integer / Q

# relative bounds per element, in units of U (derivation: module docstring of tests/test_map_loss_numerics_gpu.py)
B_COLOR = 4
B_DEPTH = 9                      # with the uncertainty weight
B_DEPTH_PLAIN = 2                # uncertainty off: sign / count
B_SDF_EXP = 22                   # front samples whose gradient is -sparse exp(-sparse pred) (a > diff, m >= 0)
B_SDF_UNIT = {"kernel": 4, "torch": 6}      # samples whose gradient is +-1 times the ray's scale
K_LOSS = 29                      # per-ray loss of the kernel: K_LOSS U sum |terms|


def k_total(path, n, s):
    """bound factor of the SCALAR loss mapping_loss_sharded returns (any summation order over its addends)"""
    return K_LOSS + n + 4 if path == "kernel" else 24 + max(3 * n, n + s)


VARIANTS = ("near_strict", "arg_strict", "no_gate", "nvs_without_front", "local_count", "uw_on_colour", "da_without_one")


def _f32(x):
    """the fp32 value the kernel receives for a host float, as a Python float (= exact in fp64)"""
    return float(np.float32(x))


def referee(c, variant=None):
    """Per-ray loss [n], d_color [n,3], d_depth [n,1], d_sdf [n,s] (autograd on the sum of the per-ray losses), and
    abs_terms [n] = the per-ray sum of the ABSOLUTE values of the loss's addends (exp(arg) - 1 counts as the two addends
    exp(arg) and 1: the device exp's error is relative to exp(arg), not to the difference), all float64.
    `variant`: one of VARIANTS = a subtly wrong loss (tests/test_map_loss_cpu.py::test_wrong_variants_miss_the_bounds)."""
    assert variant is None or variant in VARIANTS
    d = lambda k: c[k].detach().double()
    color, depth, sdf = (d(k).requires_grad_(True) for k in ("color", "depth", "sdf"))
    n, s = sdf.shape
    trunc, sparse = _f32(c["trunc"]), _f32(c["sparse"])
    w_color, w_sdf = _f32(c["w_color"]), _f32(c["w_sdf"])
    rays_depth = d("rays_depth").reshape(-1, 1)
    valid = (rays_depth > 0).reshape(-1)
    idx = valid.nonzero().reshape(-1)
    count = float(valid.sum()) if variant == "local_count" else float(c["count"])

    gt = rays_depth[valid]
    est_color, est_depth, pred, z = color[valid], depth[valid], sdf[valid], d("z_vals")[valid]
    uw = 1.0 / torch.sqrt(d("depth_variance")[valid] + 1e-10)
    if not c["uncertainty"]:
        uw = torch.ones_like(uw)
    # colour: |.|.mean() over [nv, 3]; depth: (|.| * uw).mean() over [nv, 1] -- per ray, the division by nv comes last
    col_abs = torch.abs(est_color - d("rays_color")[valid])
    if variant == "uw_on_colour":
        col_abs = col_abs * uw
    col_ray = col_abs.sum(1) / 3.0
    dep_ray = (torch.abs(est_depth - gt) * uw).reshape(-1)
    # compute_sdf_error
    front = z < (gt - trunc)
    bound = gt - z
    near = (bound.abs() < trunc) if variant == "near_strict" else (bound.abs() <= trunc)
    nvs = near.sum(1) + 1e-8
    if variant != "nvs_without_front":
        nvs = nvs + front.sum(1)
    arg = -sparse * pred
    if variant == "arg_strict":
        argc = torch.where(arg < 10.0, arg, torch.full_like(arg, 10.0))         # no gradient AT the clamp value
    else:
        argc = arg.clamp(max=10.0)
    e = torch.exp(argc)
    a = e - torch.ones_like(pred)
    if variant == "da_without_one":                   # same value; d a / d pred = -sparse (exp - 1) inside the clamp
        h = e - argc
        a = a.detach() + (h - h.detach())
    diff = pred - bound
    m = torch.max(a, diff)
    front_loss = (m if variant == "no_gate" else m.clamp(min=0.0)) * front
    sdf_ray = front_loss.sum(1) / nvs + (torch.abs(diff) * near).sum(1) / nvs
    per_valid = (w_color * col_ray + dep_ray + w_sdf * sdf_ray) / count
    loss_rays = torch.zeros(n, dtype=torch.float64).index_add(0, idx, per_valid)
    loss_rays.sum().backward()

    with torch.no_grad():
        passes = front & ((m >= 0) | (variant == "no_gate"))
        front_abs = torch.where(a > diff, e + 1.0, diff.abs()) * passes
        sdf_abs = front_abs.sum(1) / nvs + (diff.abs() * near).sum(1) / nvs
        abs_valid = (w_color * col_abs.sum(1) / 3.0 + dep_ray.abs() + w_sdf * sdf_abs) / count
        abs_terms = torch.zeros(n, dtype=torch.float64).index_add(0, idx, abs_valid)
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    return dict(loss_rays=loss_rays.detach(), d_color=zero(color), d_depth=zero(depth), d_sdf=zero(sdf),
                abs_terms=abs_terms)


def masks(c):
    """float64 masks and quantities of EVERY ray (invalid rays: all masks false), for the tests' preconditions and the
    per-element choice of bound: front, near, a, diff, m, arg [n,s]; valid [n]"""
    d = lambda k: c[k].detach().double()
    trunc, sparse = _f32(c["trunc"]), _f32(c["sparse"])
    gt = d("rays_depth").reshape(-1, 1)
    valid = gt > 0
    z, pred = d("z_vals"), d("sdf")
    bound = gt - z
    front = (z < gt - trunc) & valid
    near = (bound.abs() <= trunc) & valid
    arg = -sparse * pred
    a = torch.exp(arg.clamp(max=10.0)) - 1.0
    diff = pred - bound
    return dict(front=front, near=near, a=a, diff=diff, m=torch.max(a, diff), arg=arg, bound=bound, pred=pred,
                valid=valid.reshape(-1), exp_branch=front & (torch.max(a, diff) >= 0) & (a > diff))


def bounds(c, ref, path="kernel"):
    """per-element absolute bounds of d_color, d_depth, d_sdf and per-ray of loss_rays for one case"""
    mk = masks(c)
    sdf_rel = torch.where(mk["exp_branch"], float(B_SDF_EXP), float(B_SDF_UNIT[path]))
    return dict(d_color=B_COLOR * U * ref["d_color"].abs(),
                d_depth=(B_DEPTH if c["uncertainty"] else B_DEPTH_PLAIN) * U * ref["d_depth"].abs(),
                d_sdf=sdf_rel * U * ref["d_sdf"].abs(),
                loss_rays=K_LOSS * U * ref["abs_terms"])


def worst_ratio(got, ref, bnd):
    """max |got - ref| / bound over the elements; inf if an element with bound 0 (the referee's exact zeros) is not 0 or
    anything is not finite"""
    got = got.detach().double().cpu().reshape(ref.shape)
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    err = (got - ref).abs()
    if bool((err[bnd == 0] != 0).any()):
        return float("inf")
    pos = bnd > 0
    return float((err[pos] / bnd[pos]).max()) if bool(pos.any()) else 0.0


def total(c, ref):
    """the scalar mapping_loss_sharded returns on this shard (per-ray losses + the eikonal share) and the sum of the
    absolute values of its addends, float64"""
    n = c["sdf"].shape[0]
    eik = _f32(c["w_eikonal"]) * float(c["gradient_error"].detach().double().mean()) * (n / float(c["n_rays_global"]))
    return float(ref["loss_rays"].sum()) + eik, float(ref["abs_terms"].sum()) + abs(eik)


def d_gradient_error(c):
    n = c["sdf"].shape[0]
    return _f32(c["w_eikonal"]) * (n / float(c["n_rays_global"])) / c["gradient_error"].numel()


# ------------------------------------------------------------------------------- mapping_loss_sharded on a case ----
def run_sharded(c, device, fused, monkeypatch, model):
    """mapping_loss_sharded on one case's tensors with the all-reduce replaced by the case's global counts"""
    from go_slam_amd.neus import distributed as D
    model.sdf_truncation, model.sdf_sparse_factor = c["trunc"], c["sparse"]

    def fake_all_reduce(t, group=None):
        if t.numel() == 2:                                  # [valid rays, rays] of this shard -> of all shards
            t.copy_(torch.tensor([c["count"], c["n_rays_global"]], dtype=t.dtype))
        return t
    monkeypatch.setattr(D, "all_reduce_sum_", fake_all_reduce)
    # (a copy: on the CPU `.to` returns the case's own tensor, and marking THAT as requiring gradients made every later
    # run on another device -- the GPU tests after the CPU tests in one session -- a non-leaf without .grad)
    leaf = lambda k: c[k].detach().clone().to(device).requires_grad_(True)
    ret = {"color": leaf("color"), "depth": leaf("depth"), "depth_variance": leaf("depth_variance"), "sdf": leaf("sdf"),
           "z_vals": c["z_vals"].to(device), "gradient_error": leaf("gradient_error")}
    loss, glob = D.mapping_loss_sharded(ret, c["rays_color"].to(device), c["rays_depth"].to(device),
                                        model.compute_sdf_error, None, w_color=c["w_color"], w_sdf=c["w_sdf"],
                                        w_eikonal=c["w_eikonal"], uncertainty=c["uncertainty"], fused=fused)
    loss.backward()
    return loss.detach(), glob, ret


def check_sharded(c, loss, glob, ret, path):
    """loss, d_color, d_depth, d_sdf and d_gradient_error of one mapping_loss_sharded call against the referee"""
    ref = referee(c)
    bnd = bounds(c, ref, path)
    n, s = c["sdf"].shape
    assert ret["depth_variance"].grad is None or not bool(ret["depth_variance"].grad.any())
    ratios = {k: worst_ratio(ret[k].grad, ref["d_" + k], bnd["d_" + k]) for k in ("color", "depth", "sdf")}
    want, abs_sum = total(c, ref)
    for got in (float(loss), float(glob)):
        ratios["loss"] = max(ratios.get("loss", 0.0), abs(got - want) / (k_total(path, n, s) * U * abs_sum))
    ge = float(ret["gradient_error"].grad.double().sum())
    ratios["gradient_error"] = abs(ge - d_gradient_error(c)) / (4 * U * d_gradient_error(c))
    print(path, ratios)
    assert all(r <= 1.0 for r in ratios.values()), ratios
    return ratios


# ------------------------------------------------------------------------------------------------------------ cases ----
def _ri(g, lo, hi, shape):
    return torch.randint(lo, hi, shape, generator=g, dtype=torch.int64)


def _pick(g, shape, weights):
    w = torch.tensor(weights, dtype=torch.float64)
    return torch.multinomial(w, int(np.prod(shape)), replacement=True, generator=g).reshape(shape)


def _bnd_mixed(g, n, s):
    """gt - z in grid units: half the samples in front of the truncation band (> 164), a third inside (|.| <= 160), the
    rest behind (< -164)"""
    region = _pick(g, (n, s), [0.5, 0.3, 0.2])
    return torch.where(region == 0, _ri(g, 170, 1200, (n, s)),
                       torch.where(region == 1, _ri(g, -160, 161, (n, s)), -_ri(g, 170, 1500, (n, s))))


def _build(seed, bnd_q, trunc=0.16, invalid=(), clamp_rays=None, uncertainty=True, count=None, n_rays_global=None):
    """One case from gt - z (int64 grid units, [n,s]).  The predicted SDF of a front sample is drawn from the branches of
    max(exp(clamp(-5 pred, max=10)) - 1, pred - bnd).clamp(min=0): pred < -2 and pred == -2 (only in `clamp_rays`: their
    e^10 terms would drown the ray's other addends), pred == 0, 0 < pred < bnd (m < 0), pred > bnd (diff > 0 > a) and
    -2 < pred < 0 (a > 0 > diff); of a near-surface sample: pred == bnd, above and below."""
    g = torch.Generator().manual_seed(seed)
    n, s = bnd_q.shape
    gt_q = _ri(g, 1536, 4096, (n, 1))                                   # 1.5 .. 4
    z_q = gt_q - bnd_q
    tq = _f32(trunc) * Q
    front, near = bnd_q.double() > tq, bnd_q.abs().double() <= tq
    clamp_ok = torch.zeros(n, 1, dtype=torch.bool)
    clamp_ok[list(range(0, n, 3)) if clamp_rays is None else list(clamp_rays)] = True
    cat = _pick(g, (n, s), [1, 1, 2, 2, 2, 3])
    cat = torch.where((cat < 2) & ~clamp_ok, torch.full_like(cat, 5), cat)
    bpos = bnd_q.clamp(min=2)
    pos_below = 1 + (_ri(g, 0, 1 << 30, (n, s)) % (bpos - 1))           # 1 .. bnd - 1
    pred_front = torch.where(cat == 0, -_ri(g, 2049, 6000, (n, s)),
                 torch.where(cat == 1, torch.full((n, s), -2048),
                 torch.where(cat == 2, torch.zeros(n, s, dtype=torch.int64),
                 torch.where(cat == 3, pos_below,
                 torch.where(cat == 4, bnd_q + _ri(g, 1, 600, (n, s)), -_ri(g, 1, 2048, (n, s)))))))
    ncat = _pick(g, (n, s), [1, 1, 1])
    pred_near = bnd_q + torch.where(ncat == 0, torch.zeros(n, s, dtype=torch.int64),
                                    torch.where(ncat == 1, _ri(g, 1, 400, (n, s)), -_ri(g, 1, 400, (n, s))))
    pred_q = torch.where(front, pred_front, torch.where(near, pred_near, _ri(g, -1500, 1500, (n, s))))
    rc_q = _ri(g, 0, 1025, (n, 3))
    col_q = torch.where(_pick(g, (n, 3), [1, 3]) == 0, rc_q, _ri(g, 0, 1025, (n, 3)))
    dd_q = _ri(g, 1, 600, (n, 1)) * (2 * _ri(g, 0, 2, (n, 1)) - 1)
    dd_q[list(range(1, n, 5))] = 0                                       # depth == gt on every fifth ray
    dv_q = _ri(g, 1, 200, (n, 1))
    dv_q[list(range(0, n, 4))] = 0                                       # variance 0 (weight 1e5) on every fourth
    rays_depth = gt_q.reshape(-1).clone()
    rays_depth[list(invalid)] = 0
    f = lambda t: (t.double() / Q).float()
    n_valid = int((rays_depth > 0).sum())
    c = dict(color=f(col_q), depth=f(gt_q + dd_q), depth_variance=f(dv_q), sdf=f(pred_q), z_vals=f(z_q),
             rays_color=f(rc_q), rays_depth=f(rays_depth), gradient_error=torch.tensor([0.375]),
             trunc=trunc, sparse=5, w_color=2.0, w_sdf=2.0, w_eikonal=0.1, uncertainty=uncertainty,
             count=float(n_valid if count is None else count),
             n_rays_global=float(n if n_rays_global is None else n_rays_global),
             placed=(bnd_q.abs() == 128) if trunc == 0.125 else torch.zeros(n, s, dtype=torch.bool))
    for k in ("color", "depth", "depth_variance", "sdf", "z_vals", "rays_color", "rays_depth"):
        assert bool(((c[k].double() * Q) == (c[k].double() * Q).round()).all()) and float(c[k].abs().max()) < 8.0, k
    return c


WIDTHS = [(s, n) for s in (1, 63, 64, 65, 127, 128) for n in (1, 2, 3, 5)]


def _cases():
    g = torch.Generator().manual_seed(7)
    out = {}
    out["branches"] = _build(11, _bnd_mixed(g, 24, 72), invalid=(3, 10, 17))
    row = torch.tensor([300, 129, 128, 127, 1, 0, -1, -127, -128, -129, -300, 128, -128, 200])
    out["boundary"] = _build(12, row.repeat(6, 1), trunc=0.125, invalid=(4,), clamp_rays=(0, 1))
    out["no_samples"] = _build(13, -_ri(g, 170, 1500, (5, 72)), invalid=(2,))
    for s, n in WIDTHS:
        out[f"widths-s{s}-n{n}"] = _build(100 + 8 * s + n, _bnd_mixed(g, n, s), clamp_rays=(0,))
    out["sharded"] = _build(14, _bnd_mixed(g, 13, 72), invalid=(0, 6), count=3 * 11, n_rays_global=3 * 13)
    out["empty_shard"] = _build(15, _bnd_mixed(g, 6, 72), invalid=range(6), count=7, n_rays_global=20)
    out["no_uncertainty"] = _build(16, _bnd_mixed(g, 9, 40), invalid=(5,), uncertainty=False)
    return out


CASES = _cases()
# s = 129: one more than the kernel holds per wave; gs_mapping_loss refuses it and mapping_loss_sharded takes the torch path
TOO_WIDE = _build(17, _bnd_mixed(torch.Generator().manual_seed(8), 5, 129), invalid=(1,))
