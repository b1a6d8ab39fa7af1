"""Pins tests/neus_fwd_restatement.py (the fp64 restatement of the NeuS forward and of the colour MLP's forward and
backward) without a GPU: its values against oracle/neus_autograd.py evaluated in float64 (grid_encode_diff, mlp_diff,
the SDF layer, the NeuS alpha and the compositing of neus_forward_diff, torch.autograd for the MLP backward) -- the
oracle, with the kernel's fp16 roundings applied where the contract puts them, must lie within the restated bound of
every element; the bounds against vacuity on the scenes tests/test_neus_fwd_numerics_gpu.py runs; and deliberately
wrong variants of the restated formulas against the bounds, which they must break."""
import numpy as np
import pytest
import torch

import neus_bwd_restatement as R
import neus_fwd_restatement as F
from oracle import neus_autograd as NA
from oracle import neus_oracle as NO

RAY_REGIMES = ("soft", "one_opaque", "opaque_several", "near_one", "opaque_run", "zero", "mixed_mask", "far_z")


@pytest.fixture(scope="module")
def meta():
    return NO.grid_meta()


@pytest.fixture(scope="module")
def prm(meta):
    p = R.params(0, meta)
    rng = np.random.default_rng(50)
    p["sdf_b"] = (rng.standard_normal(32) * 0.1).astype(np.float32)
    p["mlp"] = (rng.standard_normal(10240) * 0.15).astype(np.float16)
    return p


def _inside(got, want, what):
    got = np.asarray(got, np.float64).reshape(-1)
    v, e = want.v.reshape(-1), want.e.reshape(-1)
    bad = ~(np.abs(got - v) <= e)
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {v.size} outside the bound, first "
                           f"{np.nonzero(bad)[0][0]}: {got[bad][0]} vs {v[bad][0]} +- {e[bad][0]}")


def _tight(want, what, rel):
    """the bound is small against the value (not vacuous): the median of e / (|v| + 1e-3 max |v|) <= rel (sums that
    cancel have bounds of the size of what cancelled, so the maximum says nothing)"""
    v, e = np.abs(want.v).reshape(-1), want.e.reshape(-1)
    r = float(np.median(e / (v + 1e-3 * max(float(v.max()), 1e-30))))
    assert r <= rel, f"{what}: bound / |value| up to {r:.3g} (> {rel:.3g})"


def _breaks(right, wrong, what):
    assert (np.abs(wrong.v - right.v) > right.e).any(), f"{what}: the wrong variant stays within the bounds"


# ------------------------------------------------------------------------------------------------------ colour MLP ----
def _mlp_case(n, seed, n_in=67, scale=1e-3):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, n_in)) * 0.7).astype(np.float16)
    W = (rng.standard_normal(10240) * 0.15).astype(np.float16)
    d_rgb = (rng.standard_normal((n, 3)) * scale).astype(np.float32)
    rgb = rng.random((n, 3)).astype(np.float16)
    return x, W, d_rgb, rgb


@pytest.mark.parametrize("n_in", [67, 80])
def test_mlp_forward_matches_fp64_oracle(n_in):
    x, W, _, _ = _mlp_case(513, 1, n_in)
    want = F.mlp_fwd(F.pad_rows(x, n_in), W, 3)
    ref = NA.mlp_diff(torch.tensor(x, dtype=torch.float64), torch.tensor(W, dtype=torch.float64), n_in=n_in).numpy()
    _inside(ref, want["out"], "out")
    _inside(R.h16(1.0 / (1.0 + np.exp(-ref))), want["rgb"], "rgb")
    _tight(want["out"], "out", 0.1)
    _tight(want["rgb"], "rgb", 0.02)


@pytest.mark.parametrize("with_rgb", [True, False])
def test_mlp_backward_matches_fp64_autograd(with_rgb):
    n, ls = 300, 128.0
    x, W, d_rgb, rgb = _mlp_case(n, 2, 80)
    x[:, 67:] = 1.0
    want = F.mlp_bwd(x, W, d_rgb, rgb if with_rgb else None, ls)
    X = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    P = torch.tensor(W, dtype=torch.float64, requires_grad=True)
    out = NA.mlp_diff(X, P, n_in=80)
    up = d_rgb.astype(np.float64) * ls
    if with_rgb:
        y = rgb.astype(np.float64)
        up = up * y * (1 - y)
    (out * torch.tensor(up)).sum().backward()
    _inside(X.grad.numpy(), want["dX"], "dX")
    g = P.grad.numpy()
    _inside(g[:5120], want["dW1"], "dW1")
    _inside(g[5120:9216], want["dW2"], "dW2")
    _inside(g[9216:], want["dW3"], "dW3")
    _tight(want["dX"], "dX", 0.05)


def test_mlp_wrong_variants_break_the_bounds():
    x, W, d_rgb, rgb = _mlp_case(257, 3, 80)
    X = F.pad_rows(x, 80)
    _breaks(F.mlp_fwd(X, W)["out"], F.mlp_fwd(X, W, _wrong="swap_w2_k")["out"], "W2 K fragments 1, 2 swapped")
    right, wrong = F.mlp_bwd(X, W, d_rgb, rgb, 128.0), F.mlp_bwd(X, W, d_rgb, rgb, 128.0, _wrong="mask_ge")
    _breaks(right["dX"], wrong["dX"], "[H >= 0] mask: dX")
    _breaks(right["dW1"], wrong["dW1"], "[H >= 0] mask: dW1")


# ------------------------------------------------------------------------------------------------------ ray stage ----
def _composite(sc, scale):
    """neus_forward_diff's compositing in float64"""
    t = lambda k: torch.tensor(np.asarray(sc[k], np.float64))
    a, m, z, g = t("alpha"), t("mask"), t("z_mid"), t("grad")
    rgb = torch.tensor(np.asarray(sc["rgb"], np.float16).astype(np.float64))
    n = a.shape[0]
    w = a * torch.cumprod(torch.cat([torch.ones(n, 1, dtype=torch.float64), 1 - a + 1e-7], 1), 1)[:, :-1]
    dep = (z * w).sum(1)
    gerr = ((torch.linalg.norm(g, dim=2) - 1.0) ** 2 * m).sum(1) * scale
    return {"color": (rgb * w[..., None]).sum(1), "depth": dep, "depth_var": ((z - dep[:, None]) ** 2 * w).sum(1),
            "normal": (g * w[..., None] * m[..., None]).sum(1), "weight_sum": w.sum(1), "grad_err": gerr}


@pytest.mark.parametrize("s", [1, 63, 65, 129])
@pytest.mark.parametrize("regime", RAY_REGIMES)
def test_ray_stage_matches_fp64_compositing(regime, s):
    sc = R.ray_scene(5, s, regime, seed=s)
    scale = float(np.float32(1.0 / (5 * s)))
    want = F.ray_fwd(sc["alpha"], sc["rgb"], sc["z_mid"], sc["grad"], sc["mask"], scale)
    ref = _composite(sc, scale)
    for k, x in ref.items():
        _inside(x.numpy(), want[k], f"{regime} s={s} {k}")
        if regime in ("soft", "far_z"):
            _tight(want[k], k, 5e-4 if k != "depth_var" else 0.3)


def _c7_scene(n, s):
    """sample 0 nearly opaque (1 - 2^-20) and black, the rest white: the colour is the light behind sample 0, whose
    transmittance 2^-20 + 1e-7 is 10 % more than without the 1e-7"""
    sc = R.ray_scene(n, s, "soft", seed=2)
    sc["alpha"][:, 0] = np.float32(1.0 - 2.0 ** -20)
    sc["rgb"][:] = 1.0
    sc["rgb"][:, 0] = 0.0
    return sc


def test_ray_wrong_variants_break_the_bounds():
    for s in (64, 72, 129):
        for wrong, key, sc in (("no_c7", "color", _c7_scene(4, s)), ("excl_shift", "depth", R.ray_scene(4, s, "soft")),
                               ("var_depth", "depth_var", R.ray_scene(4, s, "soft"))):
            args = (sc["alpha"], sc["rgb"], sc["z_mid"], sc["grad"], sc["mask"], 1.0)
            _breaks(F.ray_fwd(*args)[key], F.ray_fwd(*args, _wrong=wrong)[key], f"{wrong} s={s}")


def test_piece_layout_forced_points_and_sums():
    assert F.pieces(10, 4, 3) == [(0, 3), (3, 4), (4, 7), (7, 8), (8, 10)]
    m = np.zeros(10 * 7, bool)
    m[3 * 7 + 2] = True                                  # the one in-bound point of piece (3, 4)
    fm = F.forced_mask(m, 7, 10, 4, 3)
    assert fm[:21].all() and fm[21:28].sum() == 1 and fm[23] and fm[28:].all()
    big = F.forced_mask(np.zeros(300 * 2, bool), 2, 300, 300, 300)
    assert big[:100].all() and not big[100:].any()
    g = np.float32([1e-3, 2e-3, 3e-3, 1e8, -1e8, 5e-9, 1.0, 2.0, 3.0, 4.0])
    ps = F.piece_sum(g, 10, 4, 3)
    exact = np.array([sum(float(x) for x in g[a:b]) for a, b in F.pieces(10, 4, 3)])
    assert np.all(np.abs(ps[:, 0] - exact) <= 1e-9 * np.abs(exact))
    assert np.all(np.abs(np.float32(ps[:, 0]) - ps[:, 0]) <= ps[:, 1])


# ---------------------------------------------------------------------------------------------------- point stage ----
POINT_SCENES = ("soft", "hard3", "hard5", "lanes", "one")


def _oracle_points(sc, prm, meta, inv_s, live):
    """the point stage in float64 torch from oracle/neus_autograd.py's pieces, for the live points"""
    s = sc["s"]
    zv, dv = sc["z_vals"].reshape(-1), sc["dists"].reshape(-1)
    pt, qn, inside, view, span = R.positions(sc["rays_o"], sc["rays_d"], zv, dv, s, R.BOUND)
    idx = np.nonzero(live)[0]
    T = lambda x: torch.tensor(np.asarray(x, np.float64))
    enc, dydx = NA.grid_encode_diff(T(view[idx]), T(prm["grid"].astype(np.float32)), meta)
    W, b = T(prm["sdf_w"]), T(prm["sdf_b"])
    out = torch.cat([T(qn[idx]), enc], 1) @ W.t() + b
    gview = torch.einsum("ncd,c->nd", dydx, T(R.h16(prm["sdf_w"][0, 3:])))
    grad = (W[0, :3][None] + gview / 2) * T(inside[idx]) * 2.0 / T(span)
    dirs = T(sc["rays_d"])[torch.tensor(idx // s)]
    cos = (dirs * grad).sum(1)
    ic = -torch.relu(-cos)
    dist = T(dv[idx])
    sdf = out[:, 0]
    p = torch.sigmoid((sdf - ic * dist / 2) * float(inv_s))
    c = torch.sigmoid((sdf + ic * dist / 2) * float(inv_s))
    alpha = ((p - c + 1e-5) / (p + 1e-5)).clip(0.0, 1.0)
    emb = torch.sin(T(pt[idx]) @ T(prm["color_B"]))
    h = lambda x: T(R.h16(x.detach().numpy()))
    row = torch.cat([h(emb), h(grad), h(out[:, 1:]), torch.ones(idx.size, 13, dtype=torch.float64)], 1)
    aux = torch.stack([torch.cat([enc[:, 2 * l:2 * l + 2], h(dydx[:, 2 * l, :]), h(dydx[:, 2 * l + 1, :])], 1)
                       for l in range(R.LEVELS)], 0)
    return {"sdf": sdf, "grad": grad, "alpha": alpha, "mlp_in": row, "enc_aux": aux}


@pytest.mark.parametrize("name", POINT_SCENES)
def test_point_stage_matches_fp64_oracle(name, meta, prm):
    sc = R.scene(name, seed=7, meta=meta)
    live = np.ones(sc["z_vals"].size, bool)
    live[::5] = False
    want = F.point_fwd(sc["rays_o"], sc["rays_d"], sc["z_vals"], sc["dists"], sc["s"], prm["grid"], prm["sdf_w"],
                       prm["sdf_b"], prm["color_B"], sc["inv_s"], R.BOUND, live, meta)
    ref = _oracle_points(sc, prm, meta, sc["inv_s"], live)
    for k, x in ref.items():
        _inside(x.detach().numpy(), want[k], f"{name} {k}")
    if name in ("soft", "lanes"):
        _tight(want["sdf"], "sdf", 1e-3)
        _tight(want["grad"], "grad", 1e-3)
        _tight(want["mlp_in"], "mlp_in", 2e-3)


def test_point_mask_and_z_mid_are_the_fp32_chain():
    o = np.array([[2.4, 0, 0], [0, 0, 0]], np.float32)
    d = np.array([[1, 0, 0], [0, 1, 0]], np.float32)
    z = np.array([[0.0], [0.5]], np.float32)
    dist = np.array([[0.2], [0.0]], np.float32)
    zm, m = F.z_mid_mask(o, d, z, dist, 1, np.array([-2.5, 2.5, -1, 1, -1, 1], np.float32))
    assert zm.dtype == np.float32 and zm[0] == np.float32(0.1) and zm[1] == np.float32(0.5)
    assert m[0] == (np.float32(2.4) + np.float32(0.1) < np.float32(2.5))        # strict: a point on the face is out
    assert m[1]
    zm, m = F.z_mid_mask(o, d, z, dist, 1, np.array([-2.5, 2.5, 0, 1, -1, 1], np.float32))
    assert not m[0] and m[1]                                                   # y = 0 on the face y > 0: out
