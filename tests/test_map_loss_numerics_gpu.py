"""gs_mapping_loss (go_slam_amd/csrc/map_loss.hip) per element against the float64 referee of
tests/map_loss_restatement.py, on every branch of the loss: the exp clamp and its edge, m < 0 and m == 0, zero residuals,
the mask boundaries, 1..128 samples per ray, partial workgroups, rays without samples, a global count that differs from
the local one, a shard without depth, uncertainty off.  tests/test_map_loss_cpu.py shows that the cases reach those
branches with a margin and that wrong losses miss the bounds below by factors of 1e5 and more.

The kernel is called through the C ABI as `_MapLossFn.forward` calls it; the four output buffers are filled with NaN first
(plus a guard behind each), so an element that is not written fails its comparison.

Bounds.  u = 2^-24; every fp32 +, -, *, / (the compiler's default for `/` in device code is the correctly rounded
sequence) contributes a relative u; first-order counts, one extra u for the second-order terms and for the referee's
`+ 1e-8` in nvs, which fp32 absorbs (relative 1e-8 / nvs < u / 5 for nvs >= 1; for nvs = 1e-8 the numerators are exact
zeros).  The HIP math documentation is not part of the ROCm install the suite runs on, so expf and sqrtf are BUDGETED
at 2 ulp = 4 u each -- a budget, not a measurement.  The inputs are on the grid k / 1024, so every difference the signs and
masks are taken from (gt - z, pred - bnd, color - rays_color, depth - gt) is exact.

  inv_nv = 1 / counts[0]                                                              1
  d_color = ((w_color sg) inv_nv) / 3          sg = +-1 exact; *, /                    1 + 2 = 3        bound  4 u
  uw = 1 / sqrtf(dvar + 1e-10f)                1e-10f and the + : 2, halved by the root 1; sqrtf 4; /   6
  d_depth = (sgd uw) inv_nv                    6 + 1 + *                               8                bound  9 u
            uncertainty off: uw = 1 exactly    1                                                        bound  2 u
  gs_scale = (w_sdf inv_nv) / nvs              1 + * + /                               3
  d_sdf, g = +-1 (near-surface; diff > 0 > a)  g gs_scale exact                        3                bound  4 u
  d_sdf, g = da = -sparse (a + 1)              arg = -sparse pred: one rounding, amplified by |arg| <= 10 through exp: 10;
                                               expf 4: e within 14; a = e - 1: |err| <= 14 e + |a|; a + 1: + e more; this
                                               branch needs m = a >= 0, so e >= 1 and |a| <= e: a + 1 within 16 of e;
                                               * sparse 1; * gs_scale 3 + 1                                21  bound 22 u
  (arg > 10: da = 0 exactly; the tie a == diff cannot occur where m >= 0: it needs pred <= 0 and pred >= bnd > trunc.)
  all of them are below 64 u.

  loss_rays <= K u (sum over the ray's addends |t|) / counts[0], where exp(arg) - 1 is the two addends exp(arg) and 1:
    sdf:    e 14, a = e - 1 one more 15; second sample of the lane 1; wave sum 4 DPP steps + 2 levels 6; / nvs 1;
            * w_sdf 1; the two + of the three terms 2; * inv_nv 1 + 1                                   28
    colour: 2 + (three |d|), * w_color, / 3: 4; then 2 + 2                                               8
    depth:  uw 6, * 1; then 2 + 2                                                                       11
    K = 28 + 1 = 29 <= 32.

The torch path of mapping_loss_sharded (fused=False, or s > 128) is held to the same per-element bounds, except that a
+-1 sample passes five roundings there (w_sdf, nv_l / nv_g and its product, / nvr, / nvs): 6 u; its exp samples pass
1 + 2 + 1 + 1 + 15 + 1 = 21.  The SCALAR loss either path returns adds its addends in an order of torch's choosing, and N
addends cost at most N - 1 roundings in any order: fused K + (n - 1) + 5 for the sum over rays and the eikonal share;
unfused at most 15 per sample + (s - 1) + (n - 1) + 9 for the sdf term and 3 n + 7 for the colour term, taken as
24 + max(3 n, n + s) (map_loss_restatement.k_total).

Elements the referee gives as exact zeros -- invalid rays, masked samples, m < 0, diff == 0, arg > 10, an empty shard -- must
be exact zeros.  The worst error / bound ratio per output goes to $MAP_LOSS_NUMERICS_REPORT (JSON) when it is set."""
# largest error / bound seen on an MI355X: d_color 0.24, d_depth 0.24, d_sdf 0.31 (0.08 at pred == 0), loss_rays 0.09
import json
import os

import pytest
import torch

import map_loss_restatement as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
GUARD = 64
OUTS = ("d_color", "d_depth", "d_sdf", "loss_rays")

_stats = {}

assert max(R.B_COLOR, R.B_DEPTH, R.B_SDF_EXP, *R.B_SDF_UNIT.values()) < 64 and R.K_LOSS <= 32


@pytest.fixture(scope="module", autouse=True)
def _report(built_lib):
    yield
    out = os.environ.get("MAP_LOSS_NUMERICS_REPORT")
    if out:
        with open(out, "w") as f:
            json.dump(_stats, f, indent=1, sort_keys=True)


def _note(key, r):
    _stats[key] = max(_stats.get(key, 0.0), r)


@pytest.fixture(scope="module")
def model(built_lib):
    from go_slam_amd.neus import InstantNeuS
    return InstantNeuS({}, [[-1.0, 1.0]] * 3, device=DEV).to(DEV)


def _launch(c):
    """gs_mapping_loss on one case -> (status, {output: NaN-prefilled buffer with its guard})"""
    from go_slam_amd import _lib
    n, s = c["sdf"].shape
    f = lambda k: c[k].detach().float().contiguous().to(DEV)
    ins = [f(k) for k in ("color", "depth", "depth_variance", "sdf", "z_vals", "rays_color", "rays_depth")]
    counts = torch.tensor([c["count"]], dtype=torch.float32, device=DEV)
    size = dict(d_color=3 * n, d_depth=n, d_sdf=n * s, loss_rays=n)
    out = {k: torch.full((size[k] + GUARD,), NAN, dtype=torch.float32, device=DEV) for k in OUTS}
    rc = _lib.lib().gs_mapping_loss(*[_lib.ptr(t) for t in ins], _lib.ptr(counts), float(c["trunc"]), float(c["sparse"]),
                                    float(c["w_color"]), float(c["w_sdf"]), int(bool(c["uncertainty"])),
                                    *[_lib.ptr(out[k]) for k in OUTS], n, s, _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    return rc, {k: v.cpu() for k, v in out.items()}, size


def _outputs(c):
    rc, out, size = _launch(c)
    assert rc == 0
    for k in OUTS:
        assert bool(out[k][size[k]:].isnan().all()), f"{k}: written past its end"
    return {k: out[k][:size[k]] for k in OUTS}


@pytest.mark.parametrize("name", list(R.CASES))
def test_kernel_matches_the_referee_per_element(name):
    c = R.CASES[name]
    got = _outputs(c)
    ref = R.referee(c)
    bnd = R.bounds(c, ref, "kernel")
    ratios = {k: R.worst_ratio(got[k], ref[k], bnd[k]) for k in OUTS}
    print(name, ratios)
    for k in OUTS:
        _note(k, ratios[k])
    assert all(r <= 1.0 for r in ratios.values()), ratios
    if name == "empty_shard":
        for k in OUTS:
            assert bool((got[k] == 0).all()), k


def test_zero_sdf_in_front_of_the_surface_passes_minus_sparse():
    """pred == 0 in a front sample: a = exp(0) - 1 = 0 = m exactly, the clamp(min=0) passes the gradient and d_sdf is
    -sparse w_sdf / (counts[0] nvs)"""
    seen = 0
    for name in ("branches", "sharded", "no_uncertainty"):
        c = R.CASES[name]
        mk = R.masks(c)
        sel = mk["front"] & (mk["pred"] == 0)
        nvs = (mk["front"].sum(1) + mk["near"].sum(1)).double().reshape(-1, 1) + 1e-8
        want = (-R._f32(c["sparse"]) * R._f32(c["w_sdf"]) / (c["count"] * nvs)).expand_as(sel)[sel]
        got = _outputs(c)["d_sdf"].reshape(sel.shape).double()[sel]
        r = float(((got - want).abs() / (R.B_SDF_EXP * R.U * want.abs())).max())
        _note("d_sdf_at_pred_zero", r)
        assert r <= 1.0, (name, r)
        seen += int(sel.sum())
    assert seen >= 50


def test_129_samples_are_refused_without_a_write(model, monkeypatch):
    c = R.TOO_WIDE
    rc, out, _ = _launch(c)
    assert rc != 0
    assert all(bool(v.isnan().all()) for v in out.values())
    from go_slam_amd import _lib
    assert "128" in _lib.lib().gs_last_error().decode()
    # the wrapper does not reach the kernel with it: the torch formulation, within the unfused path's bounds
    r = R.check_sharded(c, *R.run_sharded(c, DEV, True, monkeypatch, model), "torch")
    _note("sharded_too_wide", max(r.values()))


@pytest.mark.parametrize("name", ["branches", "sharded", "empty_shard"])
@pytest.mark.parametrize("fused", [True, False])
def test_mapping_loss_sharded_with_global_counts(name, fused, model, monkeypatch):
    """both paths of mapping_loss_sharded on GPU tensors, the all-reduce replaced by the case's global counts"""
    c = R.CASES[name]
    loss, glob, ret = R.run_sharded(c, DEV, fused, monkeypatch, model)
    for t in (loss, glob, *(ret[k].grad for k in ("color", "depth", "sdf", "gradient_error"))):
        assert bool(torch.isfinite(t).all())
    r = R.check_sharded(c, loss, glob, ret, "kernel" if fused else "torch")
    _note("sharded_fused" if fused else "sharded_unfused", max(r.values()))
    if name == "empty_shard":
        for k in ("color", "depth", "sdf"):
            assert bool((ret[k].grad == 0).all()), k


def test_two_launches_are_bit_identical():
    c = R.CASES["branches"]
    a, b = _outputs(c), _outputs(c)
    for k in OUTS:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
