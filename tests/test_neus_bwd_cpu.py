"""Pins tests/neus_bwd_restatement.py (the fp64 restatement of the NeuS training backward's ray and point kernels) without
a GPU: its values against torch.autograd in float64 on oracle/neus_autograd.py's graph pieces (the compositing, the
point chain through get_alpha, grid_encode_diff and the SDF layer), its table indexing against oracle.neus_oracle's grid
corners, and its error bounds against vacuity on the cases tests/test_neus_bwd_numerics_gpu.py runs."""
import numpy as np
import pytest
import torch

import neus_bwd_restatement as R
from oracle import neus_autograd as NA
from oracle import neus_oracle as NO

REGIMES = ("soft", "one_opaque", "opaque_several", "near_one", "opaque_run", "zero", "mixed_mask", "far_z")


@pytest.fixture(scope="module")
def meta():
    return NO.grid_meta()


@pytest.fixture(scope="module")
def prm(meta):
    return R.params(0, meta)


@pytest.fixture
def f64():
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    yield
    torch.set_default_dtype(old)


def _ray_autograd(sc):
    """the compositing of neus_forward_diff (weights, color, depth, depth_variance, normal, weight_sum) in float64;
    gradients w.r.t. the unmasked alpha, the rgb (masked) and the grads"""
    t = lambda k: torch.tensor(np.asarray(sc[k], np.float64))
    m = t("mask")
    a = t("alpha").requires_grad_(True)
    rgb = t("rgb").requires_grad_(True)
    g = t("grad").requires_grad_(True)
    z = t("z_mid")
    n = a.shape[0]
    am = a * m
    w = am * torch.cumprod(torch.cat([torch.ones(n, 1, dtype=torch.float64), 1 - am + R.C7], 1), 1)[:, :-1]
    depth = (z * w).sum(1, keepdim=True)
    out = {"d_color": (rgb * w[:, :, None]).sum(1), "d_depth": depth[:, 0],
           "d_dvar": ((z - depth) ** 2 * w).sum(1), "d_normal": ((g * w[:, :, None]) * m[:, :, None]).sum(1),
           "d_wsum": w.sum(1)}
    L = sum((out[k] * t(k)).sum() for k in R.UPSTREAM)
    L.backward()
    return {"d_alpha": a.grad.numpy(), "d_rgb": (rgb.grad * m[:, :, None]).numpy(), "d_grad": g.grad.numpy()}


@pytest.mark.parametrize("s", [1, 2, 64, 65, 128])
@pytest.mark.parametrize("regime", REGIMES)
def test_ray_restatement_matches_autograd(regime, s):
    base = R.ray_scene(3, s, regime, seed=s)
    for which in R.UPSTREAM + ("all",):
        sc = R.only(base, which)
        got = R.ray_bwd(**sc)
        ref = _ray_autograd(sc)
        for k, v in got.items():
            err = np.abs(v.v - ref[k])
            tol = 1e-9 * np.abs(ref[k]) + 1e-3 * v.e + 1e-300
            assert np.all(err <= tol), f"{regime} s={s} {which} {k}: max err {err.max()} vs tol"


@pytest.mark.parametrize("level", [0, 3, 4, 5, 9, 15])
def test_grid_corners_match_the_oracle(meta, level):
    rng = np.random.default_rng(level)
    r = int(meta["resolution"][level])
    gi = rng.integers(0, r, (500, 3)).astype(np.uint32)
    gi[:8] = r - 1                                          # the far corner: gi + 1 == resolution
    gi[8:16] = 0
    got = R.grid_corners(meta, level, gi)
    for c in range(8):
        b = [(c >> d) & 1 for d in range(3)]
        want = NO._grid_index(meta, level, *(gi[:, d].astype(np.int64) + b[d] for d in range(3)))
        assert np.array_equal(got[:, c], want), f"level {level} corner {c}"


def _point_autograd(P, prm, meta):
    """torch.autograd (float64) of the mapper loss's per-point terms, evaluated at the kernel's saved sdf / grad"""
    on = torch.tensor(P["on"].astype(np.float64))
    grid = torch.tensor(prm["grid"].astype(np.float64), requires_grad=True)
    W = torch.tensor(P["sdf_w"], requires_grad=True)
    cB = torch.tensor(P["color_B"], requires_grad=True)
    inv_s = torch.tensor(P["inv_s"], requires_grad=True)
    view = torch.tensor(P["view"].astype(np.float64))
    enc, dydx = NA.grid_encode_diff(view, grid, meta)
    out = torch.cat([torch.tensor(P["qn"]), enc], -1) @ W.t()
    out.retain_grad()
    g_view = torch.einsum("ncd,c->nd", dydx, NA._ste_half(W[0, 3:]))
    span = torch.tensor(P["span"])
    grad_m = (W[0, :3][None] + g_view / 2) * torch.tensor(P["inside"].astype(np.float64)) * 2.0 / span
    sdf = torch.tensor(P["sdf"]) + (out[:, 0] - out[:, 0].detach())
    g = torch.tensor(P["grad"]) + (grad_m - grad_m.detach())
    alpha = NO.get_alpha(sdf[:, None], g, torch.tensor(P["dir"]), torch.tensor(P["dists"]), inv_s)[:, 0]
    dX = torch.tensor(P["dx"].v)
    emb = torch.sin(torch.tensor(P["pts"]) @ cB)
    per = (torch.tensor(P["d_alpha"]) * alpha + torch.tensor(P["d_sdf"]) * sdf
           + torch.tensor(P["gerr"]) * (torch.linalg.norm(g, dim=1) - 1.0) ** 2
           + ((torch.tensor(P["d_grad"]) + dX[:, 33:36]) * g).sum(1) + (dX[:, 36:67] * out[:, 1:]).sum(1)
           + (dX[:, 0:33] * emb).sum(1))
    (per * on).sum().backward()
    return dict(grid=grid.grad.numpy(), sdf_w=W.grad.numpy(), cB=cB.grad.numpy(), inv_s=float(inv_s.grad),
                d_sdf=out.grad[:, 0].numpy())


@pytest.mark.parametrize("name", ["soft", "hard3", "lanes", "one"])
def test_point_restatement_matches_autograd(name, meta, prm, f64):
    sc = R.scene(name, seed=3, meta=meta)
    P = R.prepare_scene(sc, prm, meta=meta)
    got = R.point_bwd(P, "f32")
    ref = _point_autograd(P, prm, meta)
    rows = got["rows"]
    live = P["on"]
    # per point d sdf (the first d_out column)
    d0 = rows["d_out"][:, 0]
    assert np.all(np.abs(d0.v - ref["d_sdf"]) <= 1e-6 * np.abs(ref["d_sdf"]) + 1e-2 * d0.e + 1e-15), name
    # table: every entry autograd touches, and nothing else
    S, B = got["table"]
    err = np.abs(S - ref["grid"])
    assert np.all(err <= 1e-6 * np.abs(ref["grid"]) + 1e-2 * B + 1e-15), f"{name}: table, max err {err.max()}"
    assert np.all(ref["grid"][~got["touched"]] == 0.0), f"{name}: autograd touches an entry the restatement does not"
    # d inv_s
    dv, db = got["d_inv_s"]
    assert abs(dv - ref["inv_s"]) <= 1e-6 * abs(ref["inv_s"]) + 1e-2 * db + 1e-15, name
    # the rows reduced as the caller reduces them: d W = d_out^T lin_in (+ colsum dw0 into row 0), d B = pts^T d_arg
    do, li, dw = rows["d_out"], rows["lin_in"], rows["dw0"]
    gW = do.v.T @ li.v
    gW[0] += dw.v.sum(0)
    bW = np.abs(do.v).T @ li.e + do.e.T @ (np.abs(li.v) + li.e)
    bW[0] += dw.e.sum(0)
    assert np.all(np.abs(gW - ref["sdf_w"]) <= 1e-6 * np.abs(ref["sdf_w"]) + bW + 1e-15), f"{name}: sdf_w"
    gB = P["pts"].T @ rows["d_arg"].v
    assert np.allclose(gB, ref["cB"], rtol=1e-6, atol=1e-12), f"{name}: color_B"
    assert np.all(live | (np.abs(do.v).sum(1) == 0)), "a masked point has a nonzero d_out row"


def _vacuity(v, e, rel=1e-4):
    """over the entries that are not small against the output's scale: the 99th percentile of bound / |value|"""
    a = np.abs(v)
    big = a >= 1e-2 * a.max() if a.size and a.max() > 0 else np.zeros_like(a, bool)
    if not big.any():
        return 0.0
    return float(np.percentile(e[big] / a[big], 99))


@pytest.mark.parametrize("name", ["soft", "lanes", "line"])      # (hard3/hard5 saturate p (1 - p): cancellation)
def test_point_bounds_are_not_vacuous(name, meta, prm):
    sc = R.scene(name, seed=5, meta=meta)
    P = R.prepare_scene(sc, prm, meta=meta)
    for mode in ("f32", "binned"):
        got = R.point_bwd(P, mode)
        for k, x in got["rows"].items():
            # (lin_in holds the fp16-rounded encoding; d_arg the hardware cosine, 4e-6 absolute)
            lim = 1e-3 if k in ("lin_in", "d_arg") else 1e-4
            assert _vacuity(x.v, x.e) < lim, f"{name} {mode} {k}"
        S, B = got["table"]
        if mode == "binned":       # entries reduced in the bins alone (fp16 atomics take k roundings, k unbounded)
            h0 = 2 * int(meta["offset"][int(np.argmax(meta["hashed"]))])
            keep = np.arange(S.size) >= h0
            keep &= got["table_k"] == 0
            S, B = S[keep], B[keep]
        lim = 1e-4 if mode == "f32" else 1e-2   # (one fp16 rounding per record, u16 = 4.9e-4; neighbours partly cancel)
        assert _vacuity(S, B) < lim, f"{name} {mode} table: {_vacuity(S, B)}"


@pytest.mark.parametrize("regime", ["soft", "one_opaque", "near_one", "mixed_mask", "far_z"])
def test_ray_bounds_are_not_vacuous(regime):
    sc = R.ray_scene(64, 72, regime, seed=9)
    got = R.ray_bwd(**sc)
    for k, x in got.items():
        if regime == "far_z" and k == "d_alpha":            # (|z| ~ 1e3: depth_var's terms cancel in dL/dw)
            continue
        lim = 1e-3 if k == "d_alpha" else 1e-4              # (d_alpha: a difference of two terms, dL/dw T - R / t)
        assert _vacuity(x.v, x.e) < lim, f"{regime} {k}: {_vacuity(x.v, x.e)}"
