"""The NeuS forward (gs_neus_forward[_segmented]) and the colour MLP (gs_mlp_forward, gs_mlp_backward) against the fp64
restatement in tests/neus_fwd_restatement.py, per element.

Every entry is called through the C ABI (ctypes).  Every output buffer is filled with a NaN sentinel (0xAB for the
mask) and has a guard region behind it that must stay untouched; every call runs twice and must give the same bits.
  point outputs   the backward's scenes soft, big (4099 x 72), hard3, hard5, lanes, soft at inv_s = 1e-6 and 1e6, big
                  under a realtime bound that cuts rays: z_mid, mask bit-exact; sdf, grad, alpha, mlp_in, enc_aux, rgb
                  within their bounds; out-of-bound points sdf = 100 and alpha, grad, rgb, the mlp_in row exactly 0.
                  Both gather orders (gs_neus_level_major_min_points 0 and 1 << 30), inv_s by value and by device
                  pointer, the realtime bound from the host and from the device: every per-point and ray output
                  bit-identical to the first run.
  ray outputs     plane scenes (zero grid: sdf = sdf_w[0, :3] . p + sdf_b[0]) -- soft, a sharp crossing (inv_s = 1e6:
                  alpha 1 behind the plane, T through the subnormals to 0), rays starting behind the plane, grazing
                  rays, inv_s = 1e-6, |z| ~ 1e3, a mixed mask -- n in {1, 3, 5, 4099} x s in {1, 2, 63, 64, 65, 72,
                  128, 129}: colour, depth, depth_var, normal, weight_sum, grad_err_ray against the restatement fed
                  with the kernel's own per-point outputs.
  force pass      gs_neus_forward_segmented with pieces that start and end inside waves and 16-flag groups, each
                  with no in-bound point or exactly one (in its first partial wave, a whole interior wave, its last
                  partial wave; one piece of 8000 x 72 points with the point beyond wave 8192): the live points
                  exactly; forced values, grad_err_ray and grad_err_piece (piece_mean) within their bounds.
  gs_mlp_forward  n in {1, 31, 32, 33, 64, 65, 4099, 262144 + 65} x n_in in {67, 80} x n_out in {1, 3, 4}: every
                  element within its bound, >= 95 % equal to the fp16 rounding of the fp64 value.
  gs_mlp_backward n in {1, 31, 33, 97, 4099, 131072 + 17} with and without rgb, and d_rgb ls in the thousands: every
                  dX element and every dW entry (fp64 sum of the partial rows) within its bound.
The worst error / bound ratio per output and the gate-exception counts are written to $NEUS_FWD_NUMERICS_REPORT (JSON)
when it is set."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import neus_bwd_restatement as R
import neus_fwd_restatement as F
from oracle import neus_oracle as NO

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
GUARD = 64
WIDE = np.array([-3.0, 3.0, -3.0, 3.0, -3.0, 3.0], np.float32)
CUT = np.array([-2.2, 2.3, -2.4, 2.1, -2.0, 2.2], np.float32)

_stats = {"ratio": {}, "gate_exceptions": {}, "bit_identical": {}}


@pytest.fixture(scope="module", autouse=True)
def _report(built_lib):
    yield
    out = os.environ.get("NEUS_FWD_NUMERICS_REPORT")
    if out:
        with open(out, "w") as f:
            json.dump(_stats, f, indent=1, sort_keys=True)


def _lib():
    from go_slam_amd import _lib as lib_mod
    return lib_mod


def _t(x):
    return torch.as_tensor(np.ascontiguousarray(x)).to(DEV).contiguous()


def _sentinel(n, dtype=torch.float32):
    if dtype == torch.uint8:
        return torch.full((n + GUARD,), 0xAB, dtype=dtype, device=DEV)
    return torch.full((n + GUARD,), NAN, dtype=dtype, device=DEV)


def _bits(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _gates(key, counts):
    for k, v in counts.items():
        _stats["gate_exceptions"][f"{key}.{k}"] = _stats["gate_exceptions"].get(f"{key}.{k}", 0) + int(v)


def _within(key, got, want, tag):
    """every element of got (numpy) within want's bound of its value; notes the worst ratio"""
    got = np.asarray(got, np.float64).reshape(-1)
    v, e = want.v.reshape(-1), want.e.reshape(-1)
    assert got.shape == v.shape, f"{tag}: {key}: shape {got.shape} vs {v.shape}"
    err = np.abs(got - v)
    bad = ~(err <= e)
    if bad.any():
        i = int(np.nonzero(bad)[0][0])
        raise AssertionError(f"{tag}: {key}: {int(bad.sum())} of {v.size} beyond the bound, first {i}: got {got[i]!r} "
                             f"want {v[i]!r} bound {e[i]!r}")
    pos = e > 0
    r = float((err[pos] / e[pos]).max()) if pos.any() else 0.0
    _stats["ratio"][key] = max(_stats["ratio"].get(key, 0.0), r)


# ------------------------------------------------------------------------------------------------- parameters ----
@pytest.fixture(scope="module")
def meta():
    return NO.grid_meta()


def _params(meta, seed=0, zero_grid=False):
    prm = R.params(seed, meta)
    rng = np.random.default_rng(seed + 50)
    prm["sdf_b"] = (rng.standard_normal(32) * 0.1).astype(np.float32)
    prm["mlp"] = (rng.standard_normal(10240) * 0.15).astype(np.float16)
    if zero_grid:
        prm["grid"] = np.zeros_like(prm["grid"])
    return prm


@pytest.fixture(scope="module")
def prm(meta):
    return _params(meta)


def _dev(prm):
    return {k: _t(prm[k]) for k in ("grid", "sdf_w", "sdf_b", "color_B", "mlp")}


# ------------------------------------------------------------------------------------------------ the forward ----
OUTS = (("color", 3, torch.float32, "ray"), ("depth", 1, torch.float32, "ray"), ("depth_var", 1, torch.float32, "ray"),
        ("normal", 3, torch.float32, "ray"), ("weight_sum", 1, torch.float32, "ray"), ("sdf", 1, torch.float32, "pt"),
        ("z_mid", 1, torch.float32, "pt"), ("grad_err", 1, torch.float32, "ray"), ("alpha", 1, torch.float32, "pt"),
        ("rgb", 3, torch.float16, "pt"), ("grad", 3, torch.float32, "pt"), ("mask", 1, torch.uint8, "pt"),
        ("mlp_in", 80, torch.float16, "pt"), ("enc_aux", 16 * 8, torch.float16, "pt"))


def _forward(sc, dp, inv_s, rt_bound, order=1 << 30, inv_dev=False, rt_dev=False, seg=None, gerr_scale=1.0):
    """one gs_neus_forward (seg = None) or gs_neus_forward_segmented (seg = (ray_batch, piece_rays)) call with every
    optional output set; returns {name: numpy} (guards checked here)"""
    lib = _lib()
    L = lib.lib()
    n, s = sc["z_vals"].shape
    N = n * s
    old = L.gs_neus_level_major_min_points(order)
    try:
        size = {"ray": n, "pt": N}
        outs = {k: _sentinel(size[kind] * w, dt) for k, w, dt, kind in OUTS}
        ins = [_t(sc[k]) for k in ("rays_o", "rays_d", "z_vals", "dists")]
        ws = torch.empty(int(L.gs_neus_forward_workspace_bytes(n, s)), dtype=torch.uint8, device=DEV)
        bh = (ctypes.c_float * 6)(*[float(x) for x in R.BOUND])
        rt = np.asarray(rt_bound, np.float32)
        # (the values the kernel must NOT use when the device copies are given)
        rth = (ctypes.c_float * 6)(*([0.0] * 6 if rt_dev else [float(x) for x in rt]))
        rtd = _t(rt) if rt_dev else None
        invd = _t(np.array([inv_s], np.float32)) if inv_dev else None
        inv_h = NAN if inv_dev else float(inv_s)
        o = outs
        head = [lib.ptr(x) for x in ins] + [lib.ptr(dp[k]) for k in ("grid", "sdf_w", "sdf_b", "color_B", "mlp")]
        mid = [lib.ptr(invd), bh, rth, lib.ptr(rtd)] + [lib.ptr(o[k]) for k in (
            "color", "depth", "depth_var", "normal", "weight_sum", "sdf", "z_mid", "grad_err", "alpha", "rgb", "grad",
            "mask", "mlp_in", "enc_aux")]
        npieces = 0
        if seg is None:
            rc = L.gs_neus_forward(*head, inv_h, *mid, float(gerr_scale), None, 0.0, n, s, lib.ptr(ws), ws.numel(),
                                   lib.stream_ptr(DEV))
        else:
            npieces = L.gs_neus_forward_pieces(n, *seg)
            o["piece"] = _sentinel(npieces)
            rc = L.gs_neus_forward_segmented(*head, inv_h, *mid, float(gerr_scale), 1, lib.ptr(o["piece"]), None, 0.0,
                                             n, s, seg[0], seg[1], lib.ptr(ws), ws.numel(), lib.stream_ptr(DEV))
        lib.check(rc, "neus_forward")
        torch.cuda.synchronize()
    finally:
        L.gs_neus_level_major_min_points(old)
    got = {}
    for k, w, dt, kind in OUTS + (("piece", 1, torch.float32, "piece"),):
        if k not in o:
            continue
        m = (npieces if kind == "piece" else size[kind]) * w
        x = o[k]
        tail = x[m:]
        if dt == torch.uint8:
            assert bool((tail == 0xAB).all()), f"{k} written past its end"
        else:
            assert bool(tail.isnan().all()), f"{k} written past its end"
        got[k] = x[:m].cpu()
    return got


def _same(a, b, tag, keys=None):
    for k in keys or a:
        assert torch.equal(_bits(a[k]), _bits(b[k])), f"{tag}: {k} differs between the runs"


def _np(got, k, w):
    return got[k].double().numpy().reshape(-1, w) if w > 1 else got[k].double().numpy()


def _check_points(sc, prm, got, meta, inv_s, live, tag):
    """per-point outputs of one forward against point_fwd for the live points (live [N] bool, the expected mask)"""
    n, s = sc["z_vals"].shape
    N = n * s
    zm, _ = F.z_mid_mask(sc["rays_o"], sc["rays_d"], sc["z_vals"], sc["dists"], s, WIDE)
    assert np.array_equal(got["z_mid"].numpy().view(np.uint32), zm.view(np.uint32)), f"{tag}: z_mid not bit-exact"
    mk = got["mask"].numpy()
    assert np.array_equal(mk, live.astype(np.uint8)), f"{tag}: mask: {int((mk != live).sum())} points differ"
    want = F.point_fwd(sc["rays_o"], sc["rays_d"], sc["z_vals"], sc["dists"], s, prm["grid"], prm["sdf_w"],
                       prm["sdf_b"], prm["color_B"], inv_s, R.BOUND, live, meta)
    _gates("points", want["gates"])
    idx = want["idx"]
    off = ~live
    sdf, alpha = _np(got, "sdf", 1), _np(got, "alpha", 1)
    grad, rgb, mi = _np(got, "grad", 3), _np(got, "rgb", 3), _np(got, "mlp_in", 80)
    assert (sdf[off] == 100.0).all(), f"{tag}: out-of-bound sdf != 100"
    for k, x in (("alpha", alpha), ("grad", grad), ("rgb", rgb), ("mlp_in", mi)):
        assert (x[off] == 0.0).all() and not np.signbit(x[off]).any(), f"{tag}: out-of-bound {k} not exactly +0"
    _within("points.sdf", sdf[idx], want["sdf"], tag)
    _within("points.grad", grad[idx], want["grad"], tag)
    _within("points.alpha", alpha[idx], want["alpha"], tag)
    _within("points.mlp_in", mi[idx], want["mlp_in"], tag)
    aux = got["enc_aux"].double().numpy().reshape(16, N, 8)
    _within("points.enc_aux", aux[:, idx], want["enc_aux"], tag)
    m = F.mlp_fwd(mi[idx], prm["mlp"])
    _within("points.rgb", rgb[idx], m["rgb"], tag)
    return want


def _check_rays(sc, got, tag, gerr_scale=1.0):
    n, s = sc["z_vals"].shape
    want = F.ray_fwd(got["alpha"].numpy().reshape(n, s), got["rgb"].numpy().reshape(n, s, 3),
                     got["z_mid"].numpy().reshape(n, s), got["grad"].numpy().reshape(n, s, 3),
                     got["mask"].numpy().reshape(n, s), gerr_scale)
    for k, w in (("color", 3), ("depth", 1), ("depth_var", 1), ("normal", 3), ("weight_sum", 1), ("grad_err", 1)):
        x = got[k].double().numpy()
        assert np.isfinite(x).all(), f"{tag}: {k} not written (or not finite)"
        _within("rays." + k, x, want[k], tag)
    return want


# -------------------------------------------------------------------------------------------- a. point outputs ----
POINT_SCENES = ("soft", "big", "hard3", "hard5", "lanes", "inv_s_1e-6", "inv_s_1e6", "cut")


def _point_scene(name, meta):
    base = {"inv_s_1e-6": "soft", "inv_s_1e6": "soft", "cut": "big"}.get(name, name)
    sc = R.scene(base, seed=7, meta=meta)
    n = sc["z_vals"].shape[0]
    sc["z_vals"] = sc["z_vals"].reshape(n, -1)
    sc["dists"] = sc["dists"].reshape(n, -1)
    inv_s = {"inv_s_1e-6": 1e-6, "inv_s_1e6": 1e6}.get(name, float(sc["inv_s"]))
    return sc, np.float32(inv_s), (CUT if name == "cut" else WIDE)


@pytest.mark.parametrize("name", POINT_SCENES)
def test_point_outputs(name, meta, prm):
    sc, inv_s, rt = _point_scene(name, meta)
    dp = _dev(prm)
    n, s = sc["z_vals"].shape
    _, live = F.z_mid_mask(sc["rays_o"], sc["rays_d"], sc["z_vals"], sc["dists"], s, rt)
    if not live.any():
        live[:100] = True
    base = _forward(sc, dp, inv_s, rt)
    _same(base, _forward(sc, dp, inv_s, rt), f"{name}: two runs")
    _check_points(sc, prm, base, meta, inv_s, live, name)
    _check_rays(sc, base, name)
    for order, inv_dev, rt_dev in ((0, False, False), (0, True, True), (1 << 30, True, False), (1 << 30, False, True)):
        tag = f"{name} order={order} inv_dev={inv_dev} rt_dev={rt_dev}"
        other = _forward(sc, dp, inv_s, rt, order=order, inv_dev=inv_dev, rt_dev=rt_dev)
        live_keys = [k for k in base if k != "enc_aux"]
        _same(base, other, tag, live_keys)
        aux_a = base["enc_aux"].view(torch.int16).reshape(16, -1, 8)[:, torch.from_numpy(live)]
        aux_b = other["enc_aux"].view(torch.int16).reshape(16, -1, 8)[:, torch.from_numpy(live)]
        assert torch.equal(aux_a, aux_b), f"{tag}: enc_aux of the live points differs"
        _stats["bit_identical"][f"{name}.grad.order{order}"] = True


# ---------------------------------------------------------------------------------------------- b. ray outputs ----
PLANE_REGIMES = ("soft", "sharp", "behind", "grazing", "inv_s_1e-6", "far_z", "mixed_mask")
RAY_SAMPLES = (1, 2, 63, 64, 65, 72, 128, 129)


def plane_scene(n, s, regime, seed=0):
    """rays through the plane x = x0 of the zero-grid SDF sdf = x - x0 (sdf_w[0, :3] = (2.5, 0, 0) on the +-2.5 bound):
    (scene dict, inv_s, realtime bound)"""
    rng = np.random.default_rng(seed)
    o = np.zeros((n, 3))
    o[:, 1:] = rng.uniform(-1.0, 1.0, (n, 2))
    d = np.zeros((n, 3))
    d[:, 0] = -1.0
    d[:, 1:] = rng.uniform(-0.2, 0.2, (n, 2))
    near, far = 0.3, 4.2
    o[:, 0] = 2.4
    inv_s, rt = np.exp(2.0), WIDE
    if regime == "sharp":
        inv_s = 1e6
    elif regime == "behind":
        o[:, 0] = -2.4
        d[:, 0] = 1.0
    elif regime == "grazing":
        o[:, 0] = rng.uniform(-0.05, 0.05, n)
        o[:, 1] = -2.4
        d[:] = 0.0
        d[:, 1] = 1.0
        d[:, 0] = rng.choice([0.0, 1e-3, -1e-3], n)
    elif regime == "inv_s_1e-6":
        inv_s = 1e-6
    elif regime == "far_z":
        o[:, 0] = 1e3
        near, far = 1e3 - 2.4, 1e3 + 2.4
    elif regime == "mixed_mask":
        rt = CUT
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    z = np.sort(rng.uniform(near, far, (n, s)), 1)
    dist = np.concatenate([np.diff(z, axis=1), np.full((n, 1), (far - near) / max(s, 1))], 1)
    sc = dict(rays_o=o.astype(np.float32), rays_d=d.astype(np.float32), z_vals=z.astype(np.float32),
              dists=dist.astype(np.float32))
    return sc, np.float32(inv_s), rt


@pytest.fixture(scope="module")
def plane_prm(meta):
    p = _params(meta, seed=3, zero_grid=True)
    p["sdf_w"][0, :3] = (2.5, 0.0, 0.0)
    p["sdf_b"][0] = 0.25
    return p


@pytest.mark.parametrize("s", RAY_SAMPLES)
@pytest.mark.parametrize("n", [1, 3, 5, 4099])
def test_ray_outputs(n, s, plane_prm):
    dp = _dev(plane_prm)
    for regime in PLANE_REGIMES:
        sc, inv_s, rt = plane_scene(n, s, regime, seed=n * 7 + s)
        tag = f"n={n} s={s} {regime}"
        got = _forward(sc, dp, inv_s, rt, gerr_scale=np.float32(1.0 / (n * s)))
        _, live = F.z_mid_mask(sc["rays_o"], sc["rays_d"], sc["z_vals"], sc["dists"], s, rt)
        if not live.any():
            live[:100] = True
        assert np.array_equal(got["mask"].numpy(), live.astype(np.uint8)), f"{tag}: mask"
        _check_rays(sc, got, tag, np.float32(1.0 / (n * s)))
        if n == 4099:
            _same(got, _forward(sc, dp, inv_s, rt, gerr_scale=np.float32(1.0 / (n * s))), f"{tag}: two runs")


# ----------------------------------------------------------------------------------------- c. force pass, pieces ----
def _force_scene(n, s, batch, piece, kinds, seed=0):
    """rays along +x from x = -3 (every point outside the realtime bound +-2.4) except one point in each piece whose
    kind is 'first' (its first partial wave), 'interior' (a whole wave inside the piece) or 'last' (its last partial
    wave); 'none': no point.  Returns (scene, the expected live mask, the chosen points)"""
    rng = np.random.default_rng(seed)
    o = np.zeros((n, 3), np.float32)
    o[:, 0] = -3.0
    o[:, 1:] = rng.uniform(-1.0, 1.0, (n, 2))
    d = np.zeros((n, 3), np.float32)
    d[:, 0] = 1.0
    z = np.zeros(n * s, np.float32)
    chosen = []
    for k, (r0, r1) in enumerate(F.pieces(n, batch, piece)):
        p0, p1 = r0 * s, r1 * s
        kind = kinds[k % len(kinds)]
        if kind == "interior" and (-(-p0 // 64) + 1) * 64 > p1:
            kind = "last"                                 # (a ragged piece too short for a whole wave)
        if kind == "none":
            continue
        if kind == "first":
            p = p0 + (((-p0) % 64) or 64) // 2
        elif kind == "interior":
            p = -(-p0 // 64) * 64 + 37
        else:
            p = p1 - 1 - ((p1 % 64) // 3)
        assert p0 <= p < p1
        z[p] = 3.0 + rng.uniform(-0.5, 0.5)
        chosen.append(p)
    sc = dict(rays_o=o, rays_d=d, z_vals=z.reshape(n, s), dists=np.full((n, s), 0.01, np.float32))
    _, m = F.z_mid_mask(o, d, sc["z_vals"], sc["dists"], s, FORCE_RT)
    assert set(np.nonzero(m)[0]) == set(chosen)
    return sc, F.forced_mask(m, s, n, batch, piece), chosen


FORCE_RT = np.array([-2.4, 2.4, -2.4, 2.4, -2.4, 2.4], np.float32)
LAYOUTS = {                      # n, s, ray_batch, piece_rays
    "pieces_259": (1000, 7, 100, 37),
    "pieces_39": (300, 3, 64, 13),
    "pieces_odd": (777, 5, 250, 61),
}


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_force_pass_pieces(layout, meta, prm):
    n, s, batch, piece = LAYOUTS[layout]
    kinds = ("none", "first", "interior", "last") if piece * s >= 192 else ("none", "first", "last")
    sc, live, chosen = _force_scene(n, s, batch, piece, kinds, seed=n)
    dp = _dev(prm)
    got = _forward(sc, dp, np.float32(7.4), FORCE_RT, seg=(batch, piece))
    mk = got["mask"].numpy().astype(bool)
    assert np.array_equal(mk, live), f"{layout}: live points: {np.nonzero(mk != live)[0][:10]}"
    assert (got["sdf"].numpy()[~live] == 100.0).all()
    _same(got, _forward(sc, dp, np.float32(7.4), FORCE_RT, seg=(batch, piece)), f"{layout}: two runs")
    _check_points(sc, prm, got, meta, np.float32(7.4), live, layout)
    gs = F.piece_mean_scale(n, s, batch, piece)
    _check_rays(sc, got, layout, gs)
    want = F.piece_sum(got["grad_err"].numpy(), n, batch, piece)
    _within("pieces.grad_err_piece", got["piece"].double().numpy(), R.E(want[:, 0], want[:, 1]), layout)


@pytest.mark.parametrize("kind", ["none", "beyond_8192_waves"])
def test_force_pass_one_large_piece(kind, prm):
    n, s = 8000, 72
    o = np.zeros((n, 3), np.float32)
    o[:, 0] = -3.0
    d = np.zeros((n, 3), np.float32)
    d[:, 0] = 1.0
    z = np.zeros(n * s, np.float32)
    p = 8300 * 64 + 11                                   # wave 8300: the flag scan's second outer trip
    if kind != "none":
        z[p] = 3.0
    sc = dict(rays_o=o, rays_d=d, z_vals=z.reshape(n, s), dists=np.full((n, s), 0.01, np.float32))
    got = _forward(sc, _dev(prm), np.float32(7.4), FORCE_RT, seg=(n, n))
    live = np.zeros(n * s, bool)
    if kind == "none":
        live[:100] = True
    else:
        live[p] = True
    mk = got["mask"].numpy().astype(bool)
    assert np.array_equal(mk, live), f"{kind}: live points {np.nonzero(mk)[0][:10]}"
    sdf = got["sdf"].numpy()
    assert (sdf[~live] == 100.0).all() and np.isfinite(sdf[live]).all() and (sdf[live] != 100.0).all()


# ----------------------------------------------------------------------------------------------- d. gs_mlp_forward ----
def _mlp_forward(x16, W, n, n_in, n_out):
    lib = _lib()
    L = lib.lib()
    out = _sentinel(n * n_out, torch.float16)
    wsb = int(L.gs_mlp_workspace_bytes(n, n_in))
    ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=DEV)
    xd, wd = _t(x16), _t(W)                              # (held until the kernel has run)
    lib.check(L.gs_mlp_forward(lib.ptr(xd), lib.ptr(wd), lib.ptr(out), n, n_in, n_out,
                               lib.ptr(ws) if wsb else None, wsb, lib.stream_ptr(DEV)), "mlp_forward")
    torch.cuda.synchronize()
    assert bool(out[n * n_out:].isnan().all()), "mlp_forward wrote past n x n_out"
    return out[:n * n_out].cpu()


@pytest.mark.parametrize("n", [1, 31, 32, 33, 64, 65, 4099, 262144 + 65])
@pytest.mark.parametrize("n_in", [67, 80])
def test_mlp_forward(n, n_in):
    rng = np.random.default_rng(n + n_in)
    x = (rng.standard_normal((n, n_in)) * 0.7).astype(np.float16)
    W = (rng.standard_normal(10240) * 0.15).astype(np.float16)
    X = F.pad_rows(x, n_in)
    want = F.mlp_fwd(X, W, 4)["out"]
    W1, W2, W3 = F.split_mlp(W)                          # fp64 with the contract's fp16 roundings of H1, H2, out
    ref = R.h16(R.h16(np.maximum(R.h16(np.maximum(X @ W1.T, 0.0)) @ W2.T, 0.0)) @ W3[:4].T)
    eq, tot = 0, 0
    for n_out in (1, 3, 4):
        got = _mlp_forward(x, W, n, n_in, n_out)
        a = _mlp_forward(x, W, n, n_in, n_out)
        assert torch.equal(_bits(got), _bits(a)), "two runs differ"
        g = got.double().numpy().reshape(n, n_out)
        _within("mlp_forward.out", g, want[:, :n_out], f"n={n} n_in={n_in} n_out={n_out}")
        eq += int(np.sum(g == ref[:, :n_out]))
        tot += g.size
    frac = eq / tot
    key = "mlp_forward.min_fraction_equal_fp16_of_fp64"
    _stats[key] = min(_stats.get(key, 1.0), frac) if tot >= 100 else _stats.get(key, 1.0)
    assert tot < 100 or frac >= 0.95, f"n={n} n_in={n_in}: only {frac:.3f} equal the fp16 rounding of the fp64 value"


def test_mfma_keeps_fp16_subnormal_operands():
    """Does v_mfma_f32_32x32x16_f16 flush fp16 subnormal operands?  Three one-path networks through gs_mlp_forward, each
    with one subnormal operand and every other product exactly representable: an input x = 2^-20 (layer 1's B operand),
    a hidden activation H1 = 2^-20 (layer 2's B operand, written by the kernel itself), a weight W1 = 2^-20 (A operand).
    Each output is 2^-10 exactly if the subnormal operand is kept, 0 if it is flushed."""
    sub = 2.0 ** -20
    assert 0 < float(np.float16(sub)) < 2.0 ** -14
    cases = {"input": (sub, 2.0 ** 10, 1.0), "hidden": (2.0 ** -10, 2.0 ** -10, 2.0 ** 10), "weight": (2.0 ** 10, sub, 1.0)}
    res = {}
    for name, (x0, w1, w2) in cases.items():
        W = np.zeros(10240, np.float16)
        W[0] = w1                     # W1[0, 0]
        W[5120] = w2                  # W2[0, 0]
        W[9216] = 1.0                 # W3[0, 0]
        x = np.zeros((64, 80), np.float16)
        x[:, 0] = x0
        got = _mlp_forward(x, W, 64, 80, 1).double().numpy()
        want = float(x0) * float(np.float16(w1)) * float(np.float16(w2))
        res[name] = float(got[0])
        assert want == 2.0 ** -10
        assert (got == want).all(), f"{name}: {got[:4]} (2^-10 kept, 0 flushed)"
    _stats["mfma_fp16_subnormals"] = {k: ("kept" if v == 2.0 ** -10 else "flushed") for k, v in res.items()}


# ---------------------------------------------------------------------------------------------- e. gs_mlp_backward ----
def _mlp_backward(X, W, d_rgb, rgb, ls):
    from go_slam_amd.neus.tcnn_compat import _pack_mlp_fragments
    lib = _lib()
    L = lib.lib()
    n = X.shape[0]
    nb = L.gs_mlp_backward_blocks(n)
    part = _sentinel(nb * 10240)
    dX = _sentinel(n * 80, torch.float16)
    wpack = _pack_mlp_fragments(_t(W))
    xd, dd = _t(X), _t(d_rgb)                            # (held until the kernel has run)
    yd = _t(rgb) if rgb is not None else None
    lib.check(L.gs_mlp_backward(lib.ptr(xd), lib.ptr(wpack), lib.ptr(dd), lib.ptr(yd), float(ls), lib.ptr(dX),
                                lib.ptr(part), n,
                                lib.stream_ptr(DEV)), "mlp_backward")
    torch.cuda.synchronize()
    assert bool(part[nb * 10240:].isnan().all()) and bool(dX[n * 80:].isnan().all()), "written past the end"
    return dX[:n * 80].cpu(), part[:nb * 10240].cpu()


def _check_mlp_bwd(n, with_rgb, scale, tag):
    rng = np.random.default_rng(100 + n % 97)
    X = (rng.standard_normal((n, 80)) * 0.5).astype(np.float16)
    X[:, 67:] = 1.0
    W = (rng.standard_normal(10240) * 0.15).astype(np.float16)
    d_rgb = (rng.standard_normal((n, 3)) * scale).astype(np.float32)
    rgb = rng.random((n, 3)).astype(np.float16) if with_rgb else None
    ls = 128.0
    dX, part = _mlp_backward(X, W, d_rgb, rgb, ls)
    dX2, part2 = _mlp_backward(X, W, d_rgb, rgb, ls)
    assert torch.equal(_bits(dX), _bits(dX2)) and torch.equal(_bits(part), _bits(part2)), f"{tag}: two runs differ"
    want = F.mlp_bwd(X, W, d_rgb, rgb, ls)
    _gates("mlp_backward", want["gates"])
    g = dX.double().numpy().reshape(n, 80)
    assert np.isfinite(g).all(), f"{tag}: dX not finite"
    _within("mlp_backward.dX", g, want["dX"], tag)
    tot = part.double().numpy().reshape(-1, 10240).sum(0)
    _within("mlp_backward.dW1", tot[:5120], want["dW1"], tag)
    _within("mlp_backward.dW2", tot[5120:9216], want["dW2"], tag)
    _within("mlp_backward.dW3", tot[9216:], want["dW3"], tag)
    return want


@pytest.mark.parametrize("n", [1, 31, 33, 97, 4099, 131072 + 17])
@pytest.mark.parametrize("with_rgb", [True, False])
def test_mlp_backward(n, with_rgb):
    _check_mlp_bwd(n, with_rgb, 1e-3, f"n={n} rgb={with_rgb}")


def test_mlp_backward_large_gradients():
    """d_rgb ls in the thousands: the fp16 dpre / dH / dX values near the top of fp16's range, none overflowing"""
    want = _check_mlp_bwd(4099, False, 10.0, "large")
    assert 1e3 < float(np.abs(want["dX"].v).max()) < 6.5e4
