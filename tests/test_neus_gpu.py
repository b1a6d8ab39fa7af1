"""GPU parity of the mapping hot path (hash-grid NeuS renderer) vs oracle/neus_oracle.py.

Tolerances: sample placement bit-exact (ray/box intersection and sorted samples);
hash indices bit-exact (checked through dense/hash KAT levels); grid features fp16-level
(atol 1 fp16 ulp of the level amplitude); dy_dx rtol 1e-4; MLP fp16-level rtol 5e-3/atol 2e-3;
full forward: sdf rtol 1e-4, alpha atol 2e-4, colour/depth atol 3e-3 (fp16 rgb), grad rtol 1e-3.
"""
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def N(built_lib):
    import go_slam_amd.neus as neus
    return neus


@pytest.fixture(scope="module")
def O():
    from oracle import neus_oracle
    return neus_oracle


def _rays(n, seed=1, zero_frac=0.1):
    g = torch.Generator().manual_seed(seed)
    o = torch.rand(n, 3, generator=g) * 4 - 2
    d = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=1)
    gt = torch.rand(n, generator=g) * 3.5 + 0.5
    gt[torch.rand(n, generator=g) < zero_frac] = 0
    return o, d, gt


def _load(model, P):
    with torch.no_grad():
        model.sdf_network.encoding.encoding.params.copy_(P["grid"])
        model.sdf_network.sdf_layer.weight.copy_(P["sdf_w"])
        model.sdf_network.sdf_layer.bias.copy_(P["sdf_b"])
        model.color_network._B.copy_(P["color_B"])
        model.color_network.network.params.copy_(P["mlp"])
        model.variance_network.variance.fill_(P["variance"])


@pytest.mark.parametrize("with_depth,perturb", [(True, True), (True, False), (False, True)])
def test_render_sample_bit_exact(N, O, dev, with_depth, perturb):
    o, d, gt = _rays(257, seed=3)
    bound = torch.tensor([[-5.0, 5.0], [-4.0, 4.5], [-3.0, 6.0]])
    g = torch.Generator().manual_seed(9)
    pr = torch.rand(24, generator=g) if perturb else None
    zr, dr = O.render_sample(o, d, gt if with_depth else None, bound, 24, 48, pr)
    R = N.Renderer(N_samples=24, N_surface=48, perturb=1.0 if perturb else 0.0)
    z, dd = R.sample(o.to(dev), d.to(dev), bound.to(dev), gt.to(dev) if with_depth else None,
                     pr.to(dev) if perturb else None)
    assert z.shape == zr.shape
    assert torch.equal(z.cpu(), zr), f"max diff {(z.cpu() - zr).abs().max()}"
    assert torch.equal(dd.cpu()[:, :-1], dr[:, :-1])
    # last column = mean over N_samples identical values of (far-near)/N_samples (render.py:149):
    # the reduction order of that mean is backend-defined, so 1-2 ulp is the meaningful bar
    torch.testing.assert_close(dd.cpu()[:, -1], dr[:, -1], rtol=3e-7, atol=0)


def test_render_sample_mono_golden_from_the_reference_renderer(N, dev):
    """The kernel against the REFERENCE's own output (tests/golden/render_sample_mono.npz: src/render.py:99-171 executed
    verbatim with configs[4]'s 48 + 24 split; rays without depth, box exits behind the camera, a batch whose depth
    maximum is below 0.001) -- no oracle in between."""
    import numpy as np
    g = {k: torch.from_numpy(v) for k, v in np.load(os.path.join(os.path.dirname(__file__), "golden",
                                                                  "render_sample_mono.npz")).items()}
    R = N.Renderer(N_samples=48, N_surface=24, perturb=1.0)
    o, d, bound, pr = (g[k].to(dev) for k in ("rays_o", "rays_d", "bound", "perturb"))
    for tag, depth in (("depth", g["gt_depth"]), ("tiny", g["gt_depth"] * 2e-4), ("nodepth", None)):
        z, dd = R.sample(o, d, bound, None if depth is None else depth.to(dev), pr)
        z, dd, zr, dr = z.cpu(), dd.cpu(), g["z_" + tag], g["dists_" + tag]
        assert z.shape == zr.shape, tag
        assert torch.equal(z.isnan(), zr.isnan()) and torch.equal(dd.isnan(), dr.isnan()), tag
        assert torch.equal(z.nan_to_num(7.0), zr.nan_to_num(7.0)), (tag, float((z - zr).abs().nan_to_num(0).max()))
        assert torch.equal(dd[:, :-1].nan_to_num(7.0), dr[:, :-1].nan_to_num(7.0)), tag
        torch.testing.assert_close(dd[:, -1], dr[:, -1], rtol=3e-7, atol=0, equal_nan=True)   # (a mean in the reference)


def test_grid_encode_matches_oracle(N, O, dev):
    P = O.make_params(2, grid_init=0.5)
    g = torch.Generator().manual_seed(4)
    x = torch.rand(500, 3, generator=g)
    x[0] = 0.0
    x[1] = 1.0                      # the far corner (resolution edge)
    x[2] = torch.tensor([0.5, 0.25, 0.125])
    enc_r, dy_r = O.grid_encode(x, P["grid"], want_grad=True)
    enc_m = N.Encoding(3, dict(otype="HashGrid")).to(dev)
    with torch.no_grad():
        enc_m.params.copy_(P["grid"])
        enc, dy = enc_m(x.to(dev), return_dy_dx=True)
    assert enc.dtype == torch.float16 and tuple(enc.shape) == (500, 32)
    # fp16 rounding of an fp32 interpolation: at most 1 ulp apart
    diff = (enc.cpu().float() - enc_r.float()).abs()
    ulp = torch.maximum(enc_r.float().abs(), torch.tensor(6e-5)) * 2 ** -10
    assert (diff <= ulp).all(), float((diff / ulp).max())
    assert (diff == 0).float().mean() > 0.999
    torch.testing.assert_close(dy.cpu(), dy_r, rtol=1e-4, atol=1e-5)


def test_grid_meta_matches_oracle(N, O):
    from go_slam_amd import _lib
    m = _lib.grid_meta()
    r = O.grid_meta()
    assert list(m.resolution) == r["resolution"].tolist()
    assert list(m.size) == r["size"].tolist()
    assert list(m.offset) == r["offset"].tolist()
    assert list(m.hashed) == r["hashed"].tolist()
    assert [float(v) for v in m.scale] == [float(v) for v in r["scale"]], "fp32 level scales must agree bit-for-bit"
    assert int(m.total) * 2 == 12599920


@pytest.mark.parametrize("n", [1, 64, 1000])
def test_mlp_matches_oracle(N, O, dev, n):
    P = O.make_params(5)
    g = torch.Generator().manual_seed(6)
    x = torch.randn(n, 67, generator=g)
    ref = O.mlp_forward(x, P["mlp"])
    net = N.Network(67, 3, dict(otype="FullyFusedMLP", activation="ReLU", output_activation="none", n_neurons=64,
                                n_hidden_layers=2)).to(dev)
    with torch.no_grad():
        net.params.copy_(P["mlp"])
        out = net(x.to(dev))
    assert out.dtype == torch.float16 and tuple(out.shape) == (n, 3)
    torch.testing.assert_close(out.cpu().float(), ref.float(), rtol=5e-3, atol=2e-3)


def test_mlp_layout_is_not_transposed(N, dev):
    """Asymmetric weights: output o must depend on W3 row o only (catches a row/col swap)."""
    net = N.Network(67, 3).to(dev)
    w = torch.zeros(64 * 80 + 64 * 64 + 16 * 64)
    W1 = w[:5120].view(64, 80); W2 = w[5120:5120 + 4096].view(64, 64); W3 = w[9216:].view(16, 64)
    W1[5, 7] = 1.0       # hidden1[5] = x[7]
    W2[9, 5] = 2.0       # hidden2[9] = 2 * hidden1[5]
    W3[1, 9] = 0.5       # out[1] = 0.5 * hidden2[9]
    with torch.no_grad():
        net.params.copy_(w)
        x = torch.zeros(3, 67)
        x[:, 7] = torch.tensor([1.0, 2.0, -1.0])
        out = net(x.to(dev)).cpu().float()
    assert torch.allclose(out[:, 1], torch.tensor([1.0, 2.0, 0.0]))
    assert out[:, 0].abs().max() == 0 and out[:, 2].abs().max() == 0


def _mlp_backward_reference(X, W, d_rgb, rgb, ls):
    """gs_mlp_backward's contract (include/goslam_neus.h) in fp32 torch with its fp16 rounding points: H1, H2, dpre, dH2,
    dH1, dX are fp16 values; every product accumulates in fp32."""
    W1, W2, W3 = W[:5120].view(64, 80).float(), W[5120:9216].view(64, 64).float(), W[9216:].view(16, 64).float()
    Xf = X.float()
    H1 = torch.relu(Xf @ W1.t()).half().float()
    H2 = torch.relu(H1 @ W2.t()).half().float()
    dpre = torch.zeros(X.shape[0], 16, device=X.device)
    dact = rgb.float() * (1 - rgb.float()) if rgb is not None else 1.0
    dpre[:, :3] = (d_rgb * dact * ls).half().float()
    dH2 = ((dpre @ W3) * (H2 > 0)).half().float()
    dH1 = ((dH2 @ W2) * (H1 > 0)).half().float()
    return (dH1 @ W1).half(), torch.cat([(dH1.t() @ Xf).reshape(-1), (dH2.t() @ H1).reshape(-1), (dpre.t() @ H2).reshape(-1)])


@pytest.mark.parametrize("n", [1, 31, 33, 97, 4099, 131072 + 17])
@pytest.mark.parametrize("with_rgb", [True, False])
def test_mlp_backward_ragged_sizes_both_block_forms(N, dev, n, with_rgb):
    """The rebuilt colour-MLP backward at sizes that end inside a 32-point block (rows past the end go to the sink), below
    and above the switch to two sub-blocks per iteration (131072 points), with and without the sigmoid derivative (`rgb`
    NULL = tcnn.Network's contract).  Random asymmetric weights: a wrong K permutation of the packed fragments, a
    transposed tile or a mis-addressed transposing read is an O(1) error in dX / dW."""
    from go_slam_amd import _lib
    from go_slam_amd.neus.tcnn_compat import _pack_mlp_fragments
    L = _lib.lib()
    g = torch.Generator().manual_seed(100 + n % 97)
    X = (torch.randn(n, 80, generator=g) * 0.5).half().to(dev)
    X[:, 67:] = 1.0
    W = (torch.randn(10240, generator=g) * 0.15).half().to(dev)
    d_rgb = (torch.randn(n, 3, generator=g) * 1e-3).to(dev)
    rgb = torch.rand(n, 3, generator=g).half().to(dev) if with_rgb else None
    nb = L.gs_mlp_backward_blocks(n)
    partial = torch.full((nb, 10240), float("nan"), device=dev)       # (every entry must be written)
    dX = torch.full((n, 80), float("nan"), dtype=torch.float16, device=dev)
    guard = torch.zeros(4096, dtype=torch.float16, device=dev)         # (allocated right behind: nothing may land past dX)
    rc = L.gs_mlp_backward(_lib.ptr(X), _lib.ptr(_pack_mlp_fragments(W)), _lib.ptr(d_rgb), _lib.ptr(rgb) if with_rgb else None,
                           128.0, _lib.ptr(dX), _lib.ptr(partial), n, _lib.stream_ptr(dev))
    _lib.check(rc, "mlp_backward")
    torch.cuda.synchronize()
    rdX, rg = _mlp_backward_reference(X, W, d_rgb, rgb, 128.0)
    gk = partial.sum(0)
    assert torch.isfinite(dX.float()).all() and torch.isfinite(gk).all() and float(guard.float().abs().max()) == 0.0

    def rel(a, b):
        return float((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-20))
    assert rel(dX, rdX) < 2e-3, rel(dX, rdX)                 # fp16 outputs of fp32-accumulated products: ~1e-5 measured
    for name, a, b in (("dW1", gk[:5120], rg[:5120]), ("dW2", gk[5120:9216], rg[5120:9216]), ("dW3", gk[9216:], rg[9216:])):
        assert rel(a, b) < 2e-3, (name, rel(a, b))


@pytest.mark.parametrize("grid_init", [1e-4, 0.3])
def test_neus_forward_matches_oracle(N, O, dev, grid_init):
    P = O.make_params(7, grid_init=grid_init, bound=((-2.5, 2.5), (-2.5, 2.5), (-2.5, 2.5)))
    P["rt_bound"] = torch.tensor([[-2.2, 2.3], [-2.4, 2.1], [-2.0, 2.2]])
    o, d, gt = _rays(300, seed=8)
    g = torch.Generator().manual_seed(10)
    z, dist = O.render_sample(o, d, gt, P["bound"], 24, 48, torch.rand(24, generator=g))
    ref = O.neus_forward(o, d, z, dist, P)
    model = N.InstantNeuS({}, P["bound"].tolist()).to(dev)
    _load(model, P)
    model.update_bound(P["rt_bound"])
    with torch.no_grad():
        out = model(o.to(dev), d.to(dev), z.to(dev), dist.to(dev))
    assert set(out) == {"color", "depth", "depth_variance", "normal", "weight_sum", "sdf_variance", "sdf", "z_vals",
                        "gradient_error"}
    c = {k: v.cpu() for k, v in out.items()}
    assert torch.equal(c["z_vals"], ref["z_vals"])
    assert torch.equal(c["sdf"] == 100.0, ref["sdf"] == 100.0), "in-bound masks must agree exactly"
    torch.testing.assert_close(c["sdf"], ref["sdf"], rtol=1e-4, atol=2e-5)
    torch.testing.assert_close(c["weight_sum"], ref["weight_sum"], rtol=0, atol=5e-4)
    torch.testing.assert_close(c["depth"], ref["depth"], rtol=0, atol=2e-3)
    torch.testing.assert_close(c["depth_variance"], ref["depth_variance"], rtol=1e-2, atol=2e-3)
    torch.testing.assert_close(c["color"], ref["color"], rtol=0, atol=4e-3)
    torch.testing.assert_close(c["normal"], ref["normal"], rtol=2e-3, atol=2e-3)
    torch.testing.assert_close(c["gradient_error"], ref["gradient_error"], rtol=2e-3, atol=1e-5)
    torch.testing.assert_close(c["sdf_variance"], ref["sdf_variance"])


def test_embedding_sine_stays_within_a_hundredth_of_an_fp16_ulp_of_libm(N, O, dev):
    """`torch.sin(view_pts @ _B)` (InstantNeuS.py:196, _B = 25 * randn): the kernel reduces the argument with a two-term
    Cody-Waite step and takes the hardware sine; the value becomes an fp16 colour-MLP input at once.  Arguments of up to
    ~1500 rad here (points up to 14 m from the origin): every stored value must be the fp16 rounding of a number within
    3e-6 of the exact sine of the SAME fp32 argument, and all but a handful are the correctly rounded fp16 itself."""
    from go_slam_amd.neus.instant_neus import _neus_forward_raw
    P = O.make_params(11, grid_init=0.3, bound=((-10.0, 10.0), (-10.0, 10.0), (-10.0, 10.0)))
    o, d, gt = _rays(256, seed=3)
    o = o * 4.0
    g = torch.Generator().manual_seed(4)
    z, dist = O.render_sample(o, d, gt, P["bound"], 24, 48, torch.rand(24, generator=g))
    model = N.InstantNeuS({}, P["bound"].tolist()).to(dev)
    _load(model, P)
    _, inv_s = model._inv_s()
    with torch.no_grad():
        saved = _neus_forward_raw(model, o.to(dev), d.to(dev), z.to(dev), dist.to(dev), inv_s, save=True)[-1]
    mask = saved["mask"].cpu().bool().reshape(-1)
    emb = saved["mlp_in"].cpu()[:, :33][mask]
    zm = z + dist / 2.0                                                 # (the kernel's own fp32 operation order)
    pts = (o[:, None, :] + d[:, None, :] * zm[..., None]).reshape(-1, 3)[mask]
    B = P["color_B"]
    arg = (pts[:, 0:1] * B[0:1] + pts[:, 1:2] * B[1:2]) + pts[:, 2:3] * B[2:3]
    assert arg.abs().max() > 800.0
    exact = torch.sin(arg.double())
    lo = (exact - 3e-6).to(torch.float16)
    hi = (exact + 3e-6).to(torch.float16)
    assert bool(((emb >= lo) & (emb <= hi)).all())
    mismatch = (emb != exact.to(torch.float16)).float().mean().item()
    assert mismatch < 0.05, mismatch                                    # a 6e-6-wide window around an fp16 rounding boundary


def test_neus_forward_matches_the_reference_module_fixture(N, O, dev):
    """The fused forward against tests/golden/neus_forward.npz = the REFERENCE's `InstantNeuS.forward` + `compute_sdf_error`
    (src/InstantNeuS.py:295-400) executed verbatim on the tcnn stand-in, same rays / samples / parameters -- the fixture the
    oracle is pinned to (tests/test_oracle_pinned.py), here without the oracle in between."""
    import numpy as np
    g = {k: torch.from_numpy(np.asarray(v)) for k, v in
         np.load(os.path.join(os.path.dirname(__file__), "golden", "neus_forward.npz")).items() if v.dtype.kind in "fiu"}
    P = O.make_params(int(g["seed"]), grid_init=0.3, bound=((-2.5, 2.5), (-2.5, 2.5), (-2.5, 2.5)))   # (parameters only)
    model = N.InstantNeuS({}, P["bound"].tolist()).to(dev)
    _load(model, P)
    model.update_bound(g["rt_bound"])
    with torch.no_grad():
        out = model(g["rays_o"].to(dev), g["rays_d"].to(dev), g["z_in"].to(dev), g["dists_in"].to(dev))
        e, f = model.compute_sdf_error(out["sdf"], out["z_vals"], g["gt_depth"].to(dev))
    c = {k: v.cpu() for k, v in out.items()}
    assert torch.equal(c["z_vals"], g["z_vals"])
    assert torch.equal(c["sdf"] == 100.0, g["sdf"] == 100.0), "in-bound masks must agree exactly"
    torch.testing.assert_close(c["sdf"], g["sdf"], rtol=1e-4, atol=2e-5)
    torch.testing.assert_close(c["weight_sum"], g["weight_sum"], rtol=0, atol=5e-4)
    torch.testing.assert_close(c["depth"], g["depth"], rtol=0, atol=2e-3)
    torch.testing.assert_close(c["depth_variance"], g["depth_variance"], rtol=1e-2, atol=2e-3)
    torch.testing.assert_close(c["color"], g["color"], rtol=0, atol=4e-3)
    torch.testing.assert_close(c["normal"], g["normal"], rtol=2e-3, atol=2e-3)
    torch.testing.assert_close(c["gradient_error"], g["gradient_error"], rtol=2e-3, atol=1e-5)
    torch.testing.assert_close(c["sdf_variance"], g["sdf_variance"])
    torch.testing.assert_close(e.cpu(), g["sdf_error"], rtol=1e-3, atol=1e-5)
    torch.testing.assert_close(f.cpu(), g["sdf_front_error"], rtol=1e-3, atol=1e-5)


@pytest.mark.parametrize("tag", ["forced", "cut", "wide"])
def test_neus_forward_degenerate_bounds_match_the_reference_module_fixture(N, O, dev, tag):
    """The fused forward on the reference module's own outputs (tests/golden/neus_forward_cases.npz) for a realtime bound
    that contains no point (first 100 forced, InstantNeuS.py:311-312), one that leaves 34 samples, and one LARGER than
    the static bound (points outside the static bound: clamped normalisation, sdf gradient zeroed)."""
    import numpy as np
    g = {k: torch.from_numpy(np.asarray(v)) for k, v in
         np.load(os.path.join(os.path.dirname(__file__), "golden", "neus_forward_cases.npz")).items()}
    P = O.make_params(int(g["seed"]), grid_init=0.3, bound=((-2.5, 2.5), (-2.5, 2.5), (-2.5, 2.5)))   # (parameters only)
    model = N.InstantNeuS({}, P["bound"].tolist()).to(dev)
    _load(model, P)
    model.update_bound(g["rt_" + tag])
    with torch.no_grad():
        out = model(g["rays_o"].to(dev), g["rays_d"].to(dev), g["z_in"].to(dev), g["dists_in"].to(dev))
    c = {k: v.cpu() for k, v in out.items()}
    ref = lambda k: g[f"{k}_{tag}"]
    assert torch.equal(c["z_vals"], ref("z_vals"))
    assert torch.equal(c["sdf"] == 100.0, ref("sdf") == 100.0), "in-bound masks must agree exactly"
    torch.testing.assert_close(c["sdf"], ref("sdf"), rtol=1e-4, atol=2e-5)
    torch.testing.assert_close(c["weight_sum"], ref("weight_sum"), rtol=0, atol=5e-4)
    torch.testing.assert_close(c["depth"], ref("depth"), rtol=0, atol=2e-3)
    torch.testing.assert_close(c["depth_variance"], ref("depth_variance"), rtol=1e-2, atol=2e-3)
    torch.testing.assert_close(c["color"], ref("color"), rtol=0, atol=4e-3)
    torch.testing.assert_close(c["normal"], ref("normal"), rtol=2e-3, atol=2e-3)
    torch.testing.assert_close(c["gradient_error"], ref("gradient_error"), rtol=2e-3, atol=1e-5)


def test_neus_forward_no_point_in_bound_forces_first_100(N, O, dev):
    """Q14 (InstantNeuS.py:311-312): realtime bound far away => first 100 points forced valid."""
    P = O.make_params(11, grid_init=0.3, bound=((-2.5, 2.5), (-2.5, 2.5), (-2.5, 2.5)))
    P["rt_bound"] = torch.tensor([[50.0, 51.0], [50.0, 51.0], [50.0, 51.0]])
    o, d, gt = _rays(8, seed=12)
    z, dist = O.render_sample(o, d, gt, P["bound"], 24, 48, None)
    ref = O.neus_forward(o, d, z, dist, P)
    model = N.InstantNeuS({}, P["bound"].tolist()).to(dev)
    _load(model, P)
    model.update_bound(P["rt_bound"])
    with torch.no_grad():
        out = model(o.to(dev), d.to(dev), z.to(dev), dist.to(dev))
    assert int((out["sdf"] != 100.0).sum()) == 100 == int((ref["sdf"] != 100.0).sum())
    torch.testing.assert_close(out["sdf"].cpu(), ref["sdf"], rtol=1e-4, atol=2e-5)
    torch.testing.assert_close(out["color"].cpu(), ref["color"], rtol=0, atol=4e-3)


def test_forward_twice_on_a_dirty_workspace(N, O, dev):
    """The forward's workspace needs no initial state (per-wave in-bound flags, every one written by its wave): a batch
    with nothing in bound (forces the first 100 points), then a normal batch, then both again on the SAME scratch
    give bit-identical results; `gradient_error` equals the oracle's mean."""
    P = O.make_params(11, grid_init=0.3, bound=((-2.5, 2.5), (-2.5, 2.5), (-2.5, 2.5)))
    far = torch.tensor([[50.0, 51.0], [50.0, 51.0], [50.0, 51.0]])
    near = torch.tensor([[-2.2, 2.3], [-2.4, 2.1], [-2.0, 2.2]])
    o, d, gt = _rays(1500, seed=12)
    z, dist = O.render_sample(o, d, gt, P["bound"], 24, 48, None)
    model = N.InstantNeuS({}, P["bound"].tolist()).to(dev)
    _load(model, P)
    args = [t.to(dev) for t in (o, d, z, dist)]
    outs = []
    with torch.no_grad():
        for rb in (far, near, far, near):
            model.update_bound(rb)
            outs.append({k: v.clone() for k, v in model(*args).items()})
    for a, b in ((0, 2), (1, 3)):
        for k in outs[a]:
            assert torch.equal(outs[a][k], outs[b][k]), k
    assert int((outs[0]["sdf"] != 100.0).sum()) == 100
    P["rt_bound"] = near
    ref = O.neus_forward(o, d, z, dist, P)
    assert outs[1]["gradient_error"].shape == ref["gradient_error"].shape == (1,)
    torch.testing.assert_close(outs[1]["gradient_error"].cpu(), ref["gradient_error"], rtol=2e-3, atol=1e-6)
    assert int((outs[1]["sdf"] != 100.0).sum()) == int((ref["sdf"] != 100.0).sum()) > 100


def _rel(a, b):
    return float((a - b).norm() / b.norm().clamp(min=1e-12))


@pytest.mark.parametrize("grad_dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("grid_init", [0.3])
def test_training_gradients_match_autograd_oracle(N, O, dev, grid_init, grad_dtype):
    """Mapper loss (reference src/mapping.py:96-132) -> gradients of every trained parameter:
    fused HIP backward vs torch.autograd on the differentiable CPU restatement, including the
    second-order path through d sdf/d x (eikonal, normals into the colour net and alpha)."""
    from oracle import neus_autograd as NA
    P = O.make_params(21, grid_init=grid_init, bound=((-2.5, 2.5), (-2.5, 2.5), (-2.5, 2.5)))
    P["rt_bound"] = torch.tensor([[-2.2, 2.3], [-2.4, 2.1], [-2.0, 2.2]])
    o, d, gt = _rays(48, seed=22)
    g = torch.Generator().manual_seed(23)
    z, dist = O.render_sample(o, d, gt, P["bound"], 24, 48, torch.rand(24, generator=g))
    col = torch.rand(48, 3, generator=g)
    # ---- oracle
    Pd = {k: (v.clone().requires_grad_(True) if k in ("grid", "sdf_w", "sdf_b", "color_B", "mlp") else v)
          for k, v in P.items()}
    Pd["variance"] = torch.tensor(0.2, requires_grad=True)
    ref_out = NA.neus_forward_diff(o, d, z, dist, Pd)
    ref_loss = NA.mapping_loss(ref_out, col, gt)
    ref_loss.backward()
    # ---- HIP
    model = N.InstantNeuS({}, P["bound"].tolist()).to(dev)
    _load(model, P)
    model.update_bound(P["rt_bound"])
    model.grid_grad_dtype = grad_dtype      # fp32 atomics, or tcnn's fp16 packed atomics with loss scale 128
    out = model(o.to(dev), d.to(dev), z.to(dev), dist.to(dev))
    loss = NA.mapping_loss({k: v for k, v in out.items()}, col.to(dev), gt.to(dev))
    loss.backward()
    torch.testing.assert_close(loss.detach().cpu(), ref_loss.detach(), rtol=2e-3, atol=1e-4)
    pairs = {
        "grid": (model.sdf_network.encoding.encoding.params.grad, Pd["grid"].grad),
        "sdf_w": (model.sdf_network.sdf_layer.weight.grad, Pd["sdf_w"].grad),
        "sdf_b": (model.sdf_network.sdf_layer.bias.grad, Pd["sdf_b"].grad),
        "color_B": (model.color_network._B.grad, Pd["color_B"].grad),
        "mlp": (model.color_network.network.params.grad, Pd["mlp"].grad),
        "variance": (model.variance_network.variance.grad.reshape(1), Pd["variance"].grad.reshape(1)),
    }
    report = {k: _rel(a.cpu().float(), b) for k, (a, b) in pairs.items()}
    for k, r in report.items():      # measured: <= 4.3e-4 (color_B), 2.1e-4 on the grid with fp16 packed atomics
        assert r < 5e-3, report


@pytest.mark.parametrize("grad_dtype", [torch.float32, torch.float16])
def test_training_gradients_match_the_reference_module_autograd_fixture(N, O, dev, grad_dtype):
    """The HIP training backward against tests/golden/neus_backward.npz = the REFERENCE's `InstantNeuS.forward`
    differentiated by its own autograd graph (autograd.grad(create_graph=True) + backward of the mapper's loss) on a
    twice-differentiable tcnn stand-in: the gradient of every trained parameter, no oracle in between."""
    import numpy as np
    from oracle import neus_autograd as NA          # (only its loss function, itself pinned by mapper_loss.npz)
    g = {k: torch.from_numpy(np.asarray(v)) for k, v in
         np.load(os.path.join(os.path.dirname(__file__), "golden", "neus_backward.npz")).items()}
    P = O.make_params(int(g["seed"]), grid_init=0.3, bound=((-2.5, 2.5), (-2.5, 2.5), (-2.5, 2.5)))   # (parameters only)
    model = N.InstantNeuS({}, P["bound"].tolist()).to(dev)
    _load(model, P)
    model.update_bound(g["rt_bound"])
    model.grid_grad_dtype = grad_dtype
    out = model(g["rays_o"].to(dev), g["rays_d"].to(dev), g["z_in"].to(dev), g["dists_in"].to(dev))
    loss = NA.mapping_loss({k: v for k, v in out.items()}, g["rays_color"].to(dev), g["gt_depth"].to(dev))
    loss.backward()
    torch.testing.assert_close(loss.detach().cpu(), g["loss"], rtol=2e-3, atol=1e-4)
    grid_ref = torch.zeros_like(P["grid"])
    grid_ref[g["g_grid_index"]] = g["g_grid_value"]
    pairs = {"grid": (model.sdf_network.encoding.encoding.params.grad, grid_ref),
             "sdf_w": (model.sdf_network.sdf_layer.weight.grad, g["g_sdf_w"]),
             "sdf_b": (model.sdf_network.sdf_layer.bias.grad, g["g_sdf_b"]),
             "color_B": (model.color_network._B.grad, g["g_color_B"]),
             "mlp": (model.color_network.network.params.grad, g["g_mlp"]),
             "variance": (model.variance_network.variance.grad.reshape(1), g["g_variance"])}
    report = {k: _rel(a.cpu().float().reshape(b.shape), b) for k, (a, b) in pairs.items()}
    assert all(r < 5e-3 for r in report.values()), report


def test_training_step_reduces_loss(N, O, dev):
    """Plain gradient descent along the fused backward's gradient decreases the mapper loss
    monotonically; then the reference's optimiser setup (AdamW + clip 35, mapping.py:55-58,135)
    runs a step with finite results."""
    from oracle import neus_autograd as NA
    P = O.make_params(31, grid_init=0.05, bound=((-2.5, 2.5), (-2.5, 2.5), (-2.5, 2.5)))
    o, d, gt = _rays(256, seed=32)
    g = torch.Generator().manual_seed(33)
    z, dist = O.render_sample(o, d, gt, P["bound"], 24, 48, torch.rand(24, generator=g))
    col = torch.rand(256, 3, generator=g).to(dev)
    model = N.InstantNeuS({}, P["bound"].tolist()).to(dev)
    _load(model, P)
    params = model.get_training_parameters() + model.get_volume_parameters()
    args = [t.to(dev) for t in (o, d, z, dist)]
    opt = torch.optim.SGD(params, lr=1e-4)
    losses = []
    for _ in range(6):
        opt.zero_grad()
        loss = NA.mapping_loss(model(*args), col, gt.to(dev))
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
    assert losses[-1] < 0.99 * losses[0], losses
    opt = torch.optim.AdamW([{"params": model.get_training_parameters(), "lr": 1e-3},
                             {"params": model.get_volume_parameters(), "lr": 1e-2}],
                            betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    opt.zero_grad()
    loss = NA.mapping_loss(model(*args), col, gt.to(dev))
    loss.backward()
    gn = torch.nn.utils.clip_grad_norm_(params, 35.0)
    opt.step()
    assert math.isfinite(float(gn)) and all(torch.isfinite(p).all() for p in params)


def test_quirk_q15_static_bound_normalisation_with_clamp(N, O, dev):
    """Q15 (InstantNeuS.py:12-32,310,317): points are normalised with the STATIC bound and clamped to
    [-1,1] while the in-bound mask uses the REALTIME bound.  With a realtime bound larger than the
    static one, points outside the static box are encoded at the clamped position and their SDF
    gradient is zero along the clamped axis."""
    P = O.make_params(71, grid_init=0.3, bound=((-1.0, 1.0), (-1.0, 1.0), (-1.0, 1.0)))
    P["rt_bound"] = torch.tensor([[-3.0, 3.0], [-3.0, 3.0], [-3.0, 3.0]])
    o, d, gt = _rays(64, seed=72)
    z, dist = O.render_sample(o, d, gt, P["rt_bound"], 24, 48, None)
    ref = O.neus_forward(o, d, z, dist, P)
    assert (ref["_grad"].abs().sum(-1) == 0).float().mean() < 0.5 and (ref["_grad"] == 0).any()
    model = N.InstantNeuS({}, P["bound"].tolist()).to(dev)
    _load(model, P)
    model.update_bound(P["rt_bound"])
    with torch.no_grad():
        out = model(o.to(dev), d.to(dev), z.to(dev), dist.to(dev))
    torch.testing.assert_close(out["sdf"].cpu(), ref["sdf"], rtol=1e-4, atol=2e-5)
    torch.testing.assert_close(out["normal"].cpu(), ref["normal"], rtol=2e-3, atol=2e-3)
    torch.testing.assert_close(out["gradient_error"].cpu(), ref["gradient_error"], rtol=2e-3, atol=1e-5)


def test_zero_rays_are_a_noop(N, dev):
    R = N.Renderer(N_samples=24, N_surface=48)
    model = N.InstantNeuS({}, [[-2.5, 2.5]] * 3).to(dev)
    z = lambda *s: torch.zeros(*s, device=dev)
    zv, dd = R.sample(z(0, 3), z(0, 3), model.bound, z(0))
    assert tuple(zv.shape) == (0, 72) and tuple(dd.shape) == (0, 72)
    with torch.no_grad():
        out = model(z(0, 3), z(0, 3), zv, dd)
    assert tuple(out["color"].shape) == (0, 3) and tuple(out["sdf"].shape) == (0, 72)


def test_fused_mapping_loss_matches_torch_formulation(N, dev):
    """gs_mapping_loss (value + analytic gradients) vs the masked-sum PyTorch formulation of the mapper's loss
    (src/mapping.py:96-132) under autograd: rays without depth, samples in front of / around / behind the surface."""
    from go_slam_amd.neus.distributed import mapping_loss_sharded
    g = torch.Generator().manual_seed(61)
    n, s = 301, 72
    model = N.InstantNeuS({}, [[-2.5, 2.5]] * 3).to(dev)
    gt = torch.rand(n, generator=g) * 3 + 0.5
    gt[torch.rand(n, generator=g) < 0.2] = 0.0
    z = torch.sort(torch.rand(n, s, generator=g) * 4.5, dim=1).values
    z[:, 30:60] = (gt.clamp(min=0.3)[:, None] + (torch.rand(n, 30, generator=g) - 0.5) * 0.3)   # samples near the surface
    col = torch.rand(n, 3, generator=g)
    mk = lambda t: t.to(dev).requires_grad_(True)
    res = {}
    for fused in (True, False):
        ret = {"color": mk(torch.rand(n, 3, generator=torch.Generator().manual_seed(62))),
               "depth": mk(torch.rand(n, 1, generator=torch.Generator().manual_seed(63)) * 4),
               "depth_variance": mk(torch.rand(n, 1, generator=torch.Generator().manual_seed(64)) * 0.1),
               "sdf": mk(torch.randn(n, s, generator=torch.Generator().manual_seed(65)) * 0.2),
               "z_vals": z.to(dev), "gradient_error": mk(torch.tensor([0.37]))}
        loss, glob = mapping_loss_sharded(ret, col.to(dev), gt.to(dev), model.compute_sdf_error, None, fused=fused)
        loss.backward()
        res[fused] = (loss.detach(), ret["color"].grad, ret["depth"].grad, ret["sdf"].grad, ret["gradient_error"].grad,
                      ret["depth_variance"].grad)
    a, b = res[True], res[False]
    torch.testing.assert_close(a[0], b[0], rtol=1e-5, atol=1e-6)
    for i, name in ((1, "d_color"), (2, "d_depth"), (3, "d_sdf"), (4, "d_gerr")):
        torch.testing.assert_close(a[i], b[i], rtol=1e-4, atol=1e-8, msg=lambda m, nm=name: f"{nm}: {m}")
    assert a[5] is None or not bool(a[5].any())          # the uncertainty weight is detached in both


@pytest.mark.parametrize("fused", [True, False])
def test_mapping_loss_matches_the_reference_mapper_fixture(N, dev, fused):
    """gs_mapping_loss (fused = True: value + analytic gradients in one launch) and the masked-sum torch formulation
    (fused = False) against tests/golden/mapper_loss.npz = the REFERENCE's `Mapper.optimize_map` loss (src/mapping.py:96-132
    with InstantNeuS.compute_sdf_error) and the gradients its backward() left on the renderer's outputs -- rays without
    depth, zero depth variances (uncertainty weight 1e5)."""
    import numpy as np
    from go_slam_amd.neus.distributed import mapping_loss_sharded
    g = {k: torch.from_numpy(np.asarray(v)) for k, v in
         np.load(os.path.join(os.path.dirname(__file__), "golden", "mapper_loss.npz")).items()}
    model = N.InstantNeuS({}, [[-2.5, 2.5]] * 3).to(dev)
    assert model.sdf_truncation == 0.16 and model.sdf_sparse_factor == 5
    leaf = lambda k: g[k].to(dev).requires_grad_(True)
    ret = {"color": leaf("color"), "depth": leaf("depth"), "depth_variance": leaf("depth_variance"), "sdf": leaf("sdf"),
           "z_vals": g["z_vals"].to(dev), "gradient_error": leaf("gradient_error")}
    wc, ws, we = (float(x) for x in g["weights"])
    loss, glob = mapping_loss_sharded(ret, g["rays_color"].to(dev), g["rays_depth"].to(dev), model.compute_sdf_error,
                                      None, w_color=wc, w_sdf=ws, w_eikonal=we, uncertainty=True, fused=fused)
    loss.backward()
    torch.testing.assert_close(loss.detach().float().cpu(), g["loss"], rtol=2e-5, atol=1e-6)
    torch.testing.assert_close(glob.float().cpu(), g["loss"], rtol=2e-5, atol=1e-6)
    for k in ("color", "depth", "sdf", "gradient_error"):
        torch.testing.assert_close(ret[k].grad.cpu(), g["d_" + k], rtol=1e-4, atol=1e-8, msg=lambda m, k=k: f"d_{k}: {m}")
    assert ret["depth_variance"].grad is None or not bool(ret["depth_variance"].grad.any())


def _trainer_pair(N, O, dev, n_rays, seed):
    P = O.make_params(seed, grid_init=0.05, bound=((-2.5, 2.5), (-2.5, 2.5), (-2.5, 2.5)))
    o, d, gt = _rays(n_rays, seed=seed + 1)
    g = torch.Generator().manual_seed(seed + 2)
    col = torch.rand(n_rays, 3, generator=g)
    pr = torch.rand(24, generator=g)
    out = []
    from go_slam_amd.neus.mapper import MapTrainer
    for fused in (False, True):
        model = N.InstantNeuS({}, P["bound"].tolist()).to(dev)
        _load(model, P)
        out.append((model, MapTrainer(model, N.Renderer(N_samples=24, N_surface=48), fused=fused)))
    return out, [t.to(dev) for t in (o, d, col, gt, pr)]


def test_fused_mapper_step_matches_autograd_step(N, O, dev):
    """MapTrainer.step_fused (no autograd graph: loss kernel's analytic output gradients -> HIP backward -> flat-buffer
    clip + AdamW in two launches, fp16 table gradient consumed as is) vs the autograd path + clip_grad_norm_ +
    torch.optim.AdamW on two identical models: same loss and, after 4 steps, the same parameters."""
    pair, args = _trainer_pair(N, O, dev, 512, 51)
    (m_ref, t_ref), (m_fus, t_fus) = pair
    assert t_fus.fused and not t_ref.fused
    # gradients first: autograd on the reference-style loss vs the no-autograd pipeline, same parameters
    R = N.Renderer(N_samples=24, N_surface=48)
    z, dd = R.sample(args[0], args[1], m_ref.bound, args[3], args[4])
    from go_slam_amd.neus.distributed import mapping_loss_sharded
    loss_a, _ = mapping_loss_sharded(R.eval_points(args[0], args[1], z, dd, m_ref, None), args[2], args[3],
                                     m_ref.compute_sdf_error)
    loss_a.backward()
    loss_f, grid16, inv_scale = t_fus.fused_gradients(*args)
    torch.testing.assert_close(loss_f.float().cpu(), loss_a.detach().float().cpu(), rtol=2e-4, atol=1e-5)
    ref_g = {"grid": m_ref.sdf_network.encoding.encoding.params.grad, "mlp": m_ref.color_network.network.params.grad,
             "sdf_w": m_ref.sdf_network.sdf_layer.weight.grad, "sdf_b": m_ref.sdf_network.sdf_layer.bias.grad,
             "cB": m_ref.color_network._B.grad, "var": m_ref.variance_network.variance.grad}
    rep = {"grid": _rel(grid16.float().cpu() * inv_scale, ref_g["grid"].cpu())}
    for k in ("mlp", "sdf_w", "sdf_b", "cB", "var"):
        rep[k] = _rel(t_fus.flat.dense_grad(k).cpu(), ref_g[k].reshape(-1).cpu())
    assert all(v < 1e-4 for v in rep.values()), rep
    for p_ in m_ref.parameters():
        p_.grad = None
    for it in range(4):
        l_ref = t_ref.step(*args)
        l_fus = t_fus.step(*args)
        torch.testing.assert_close(l_fus.float().cpu(), l_ref.float().cpu(), rtol=2e-4, atol=1e-5,
                                   msg=lambda m: f"iteration {it}: {m}")
    names = ["sdf_network.encoding.encoding.params", "sdf_network.sdf_layer.weight", "sdf_network.sdf_layer.bias",
             "color_network._B", "color_network.network.params", "variance_network.variance"]
    pr, pf = dict(m_ref.named_parameters()), dict(m_fus.named_parameters())
    for k in names:
        a, b = pf[k].detach().float().cpu(), pr[k].detach().float().cpu()
        if k.endswith("encoding.params"):
            # The table gradient is accumulated with fp16 atomics, whose order is not reproducible: two runs of the SAME
            # path differ in ~1 % of the non-zero entries by one fp16 ulp (tools/debug_fused_mapper.py).  Adam normalises
            # every gradient to a step of +-lr, so an entry whose contributions cancel to rounding noise can take
            # opposite steps in two runs.  Measured: 0.04 % of the entries after 4 steps, each within 4 steps x lr.
            d = (a - b).abs()
            off = d > (2e-5 + 2e-3 * b.abs())
            assert float(off.float().mean()) < 2e-3 and float(d.max()) <= 4 * 1e-2 * 1.01, (float(off.float().mean()), float(d.max()))
        else:       # the dense parameters see the table's run-to-run differences through the next forward; an entry
            d = (a - b).abs()                                          # with a near-zero gradient can flip its +-lr step
            off = d > (3e-4 + 5e-3 * b.abs())
            assert float(off.float().mean()) < 2e-3 and float(d.max()) <= 4 * 1e-3 * 1.01, (k, float(off.float().mean()), float(d.max()))
    # the fused step keeps the modules usable: state_dict, inference forward with the refreshed fp16 copies
    sd = m_fus.state_dict()
    assert sd["sdf_network.encoding.encoding.params"].data_ptr() == t_fus.flat.P.data_ptr()
    with torch.no_grad():
        z, dd = N.Renderer(N_samples=24, N_surface=48).sample(args[0], args[1], m_fus.bound, args[3], args[4])
        a = m_fus(args[0], args[1], z, dd)
        b = m_ref(args[0], args[1], z, dd)
    # (the few table entries that took opposite +-lr steps above move the SDF of the samples that touch them)
    d = (a["sdf"] - b["sdf"]).abs()
    off = d > (5e-4 + 5e-3 * b["sdf"].abs())
    assert float(off.float().mean()) < 2e-3 and float(d.max()) < 1e-2, (float(off.float().mean()), float(d.max()))


def test_flat_adamw_kernels_match_torch_adamw(N, dev, built_lib):
    """gs_map_grad_sqnorm + gs_map_adamw on synthetic gradients vs clip_grad_norm_ + torch.optim.AdamW (two groups)."""
    from go_slam_amd import _lib
    g = torch.Generator().manual_seed(77)
    n16, n32 = 4096 * 8, 1003
    p = torch.randn(n16 + n32, generator=g).to(dev)
    g16 = (torch.randn(n16, generator=g) * 40).half().to(dev)           # loss-scaled by 128
    g32 = torch.randn(n32, generator=g).to(dev) * 30
    pa, pb = torch.nn.Parameter(p[:n16].clone()), torch.nn.Parameter(p[n16:].clone())
    opt = torch.optim.AdamW([{"params": [pb], "lr": 1e-3}, {"params": [pa], "lr": 1e-2}], betas=(0.9, 0.999), eps=1e-8,
                            weight_decay=0.01)
    P, M, V = p.clone(), torch.zeros_like(p), torch.zeros_like(p)
    P16 = torch.zeros(n16 + n32, dtype=torch.float16, device=dev)
    sq = torch.zeros(1, device=dev)
    L = _lib.lib()
    for step in range(1, 4):
        pa.grad, pb.grad = g16.float() / 128.0, g32.clone()
        torch.nn.utils.clip_grad_norm_([pa, pb], 35.0)
        opt.step()
        sq.zero_()
        _lib.check(L.gs_map_grad_sqnorm(_lib.ptr(g16), n16, 1 / 128.0, _lib.ptr(g32), n32, _lib.ptr(sq),
                                        _lib.stream_ptr(dev)), "sqnorm")
        _lib.check(L.gs_map_adamw(_lib.ptr(P), _lib.ptr(M), _lib.ptr(V), _lib.ptr(P16), _lib.ptr(g16), n16, 1 / 128.0,
                                  _lib.ptr(g32), n16 + n32, 1e-2, 1e-3, 0.9, 0.999, 1e-8, 0.01, step, _lib.ptr(sq), 35.0,
                                  _lib.stream_ptr(dev)), "adamw")
        ref = torch.cat([pa.detach(), pb.detach()])
        torch.testing.assert_close(P, ref, rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(P16.float(), ref.half().float(), rtol=0, atol=1e-3)
    want = float(torch.cat([g16.float() / 128.0, g32]).pow(2).sum())
    assert abs(float(sq) - want) / want < 1e-4 and want ** 0.5 > 35.0, "the clip must be active in this test"


def test_graph_replay_matches_eager_fused_step(N, O, dev):
    """MapTrainer(graph=True): the fused step captured once per batch shape in a hipGraph and replayed (static input
    buffers, device-side step count for Adam's bias corrections, perturbation vector drawn outside the graph) vs the
    same step launched eagerly on an identical model: same loss every iteration and the same parameters afterwards --
    with NEW rays in every iteration, so a replay that read stale inputs would show."""
    from go_slam_amd.neus.mapper import MapTrainer
    P = O.make_params(61, grid_init=0.05, bound=((-2.5, 2.5), (-2.5, 2.5), (-2.5, 2.5)))
    trainers = []
    for graph in (False, True):
        model = N.InstantNeuS({}, P["bound"].tolist()).to(dev)
        _load(model, P)
        trainers.append((model, MapTrainer(model, N.Renderer(N_samples=24, N_surface=48), graph=graph)))
    (m_e, t_e), (m_g, t_g) = trainers
    assert t_e.fused and t_g.fused and t_g.graph and not t_e.graph
    g = torch.Generator().manual_seed(62)
    for it in range(6):
        o, d, gt = _rays(768, seed=100 + it)
        col = torch.rand(768, 3, generator=g)
        pr = torch.rand(24, generator=g)
        args = [t.to(dev) for t in (o, d, col, gt, pr)]
        l_e, l_g = t_e.step(*args), t_g.step(*args)
        torch.testing.assert_close(l_g.float().cpu(), l_e.float().cpu(), rtol=3e-4, atol=1e-5,
                                   msg=lambda m: f"iteration {it}: {m}")
    ent = next(iter(t_g._graphs.values()))
    assert ent["graph"] is not None, "the step was never captured"
    assert t_g.flat.steps == t_e.flat.steps == 6 and int(t_g.flat.step_dev) == 6
    pe, pg = t_e.flat.P, t_g.flat.P
    d = (pe - pg).abs()
    # fp16-atomic order noise -> +-lr flips of entries whose gradient is at rounding level (see the autograd-step test):
    # ~0.06 % of the entries per step (measured 0.35 % after these 6), each by at most steps x lr
    off = d > (2e-5 + 2e-3 * pe.abs())
    assert float(off.float().mean()) < 1e-2 and float(d.max()) <= 6 * 1e-2 * 1.01, (float(off.float().mean()), float(d.max()))
    # a second batch shape gets its own graph; changing the learning rate re-captures instead of replaying stale scalars
    o, d, gt = _rays(256, seed=300)
    args2 = [t.to(dev) for t in (o, d, torch.rand(256, 3), gt)]
    for _ in range(4):
        t_g.step(*args2)
    assert len(t_g._graphs) == 2
    t_g.optimizer.set_lr(grid_lr=5e-3)
    for _ in range(3):
        t_g.step(*args2)
    assert len(t_g._graphs) == 3 and t_g.optimizer.param_groups[1]["lr"] == 5e-3


def _one_gpu_rank(rank, world, port, out):
    import os
    import torch.distributed as dist
    from go_slam_amd.neus.mapper import MapTrainer
    import go_slam_amd.neus as neus
    from oracle import neus_oracle as NO
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    dev = torch.device("cuda:0")
    P = NO.make_params(71, grid_init=0.05, bound=((-2.5, 2.5), (-2.5, 2.5), (-2.5, 2.5)))
    model = neus.InstantNeuS({}, P["bound"].tolist()).to(dev)
    _load(model, P)
    tr = MapTrainer(model, neus.Renderer(N_samples=24, N_surface=48), rank=rank, world=world)
    o, d, gt = _rays(600, seed=72)
    g = torch.Generator().manual_seed(73)
    args = [t.to(dev) for t in (o, d, torch.rand(600, 3, generator=g), gt, torch.rand(24, generator=g))]
    for _ in range(4):
        loss = tr.step(*args)
    sd = {k: v.detach().cpu() for k, v in tr.state_dict().items()}
    torch.cuda.synchronize()
    if rank == 0:
        torch.save({"loss": float(loss), "sd": sd, "slice": tr.flat.slice, "graphs": len(tr._graphs)}, out)
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_fused_step_two_ranks_on_one_gpu_equals_single_process(N, O, dev, tmp_path):
    """The sharded mapper step with the real HIP kernels: 2 ranks (both on cuda:0, gloo carrying the collectives -- RCCL
    needs one device per rank) render half the rays each, reduce-scatter the fp16 table gradient, step their slice,
    all-gather the fp16 table; 4 iterations (2 eager + capture + replay) == the single-process trainer."""
    import torch.multiprocessing as mp
    from go_slam_amd.neus.mapper import MapTrainer
    out = str(tmp_path / "two.pt")
    mp.start_processes(_one_gpu_rank, args=(2, 29800 + (os.getpid() % 1000), out), nprocs=2, join=True, start_method="spawn")
    got = torch.load(out)
    P = O.make_params(71, grid_init=0.05, bound=((-2.5, 2.5), (-2.5, 2.5), (-2.5, 2.5)))
    model = N.InstantNeuS({}, P["bound"].tolist()).to(dev)
    _load(model, P)
    tr = MapTrainer(model, N.Renderer(N_samples=24, N_surface=48))
    o, d, gt = _rays(600, seed=72)
    g = torch.Generator().manual_seed(73)
    args = [t.to(dev) for t in (o, d, torch.rand(600, 3, generator=g), gt, torch.rand(24, generator=g))]
    for _ in range(4):
        loss = tr.step(*args)
    assert got["slice"] * 2 >= tr.flat.n16 and got["graphs"] == 1
    assert abs(got["loss"] - float(loss)) < 3e-4 * max(1.0, abs(float(loss)))
    trained = {"sdf_network.encoding.encoding.params", "sdf_network.sdf_layer.weight", "sdf_network.sdf_layer.bias",
               "color_network._B", "color_network.network.params", "variance_network.variance"}
    for k, v in tr.state_dict().items():
        if k not in trained:            # (sdf_network.encoding._B is drawn at construction and never trained)
            continue
        a, b = got["sd"][k].float(), v.detach().cpu().float()
        dlt = (a - b).abs()
        lr = 1e-2 if k.endswith("encoding.params") else 1e-3
        off = dlt > (2e-5 + 2e-3 * b.abs())         # (a handful of +-lr flips of rounding-level gradients per parameter group)
        assert float(off.float().mean()) < 1e-2 and float(dlt.max()) <= 4 * lr * 1.01, (k, float(off.float().mean()), float(dlt.max()))


def _one_gpu_rank_gradients(rank, world, port, out):
    """one rank of the pre-optimiser comparison: its shard's table gradient, then exactly the step's two gradient
    collectives (FlatAdamW.step: reduce-scatter of the fp16 table gradient, all-reduce of the fp32 dense gradients)"""
    import os
    import torch.distributed as dist
    from go_slam_amd.neus.mapper import MapTrainer
    from go_slam_amd.neus.distributed import all_reduce_sum_, reduce_scatter_sum_
    import go_slam_amd.neus as neus
    from oracle import neus_oracle as NO
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    dev = torch.device("cuda:0")
    P = NO.make_params(171, grid_init=0.05, bound=((-2.5, 2.5), (-2.5, 2.5), (-2.5, 2.5)))
    model = neus.InstantNeuS({}, P["bound"].tolist()).to(dev)
    _load(model, P)
    tr = MapTrainer(model, neus.Renderer(N_samples=24, N_surface=48), rank=rank, world=world)
    n = 4096 * world
    o, d, gt = _rays(n, seed=172)
    g = torch.Generator().manual_seed(173)
    args = [t.to(dev) for t in (o, d, torch.rand(n, 3, generator=g), gt, torch.rand(24, generator=g))]
    _, g16, inv_scale = tr.fused_gradients(*args)
    flat = tr.flat
    local = flat.G16.clone()
    reduce_scatter_sum_(flat.g16s, flat.G16, None)
    all_reduce_sum_(flat.g32, None)
    torch.cuda.synchronize()
    torch.save({"local": local.cpu(), "slice": flat.g16s.cpu(), "lo": flat.lo, "hi": flat.hi, "inv_scale": inv_scale,
                "g32": flat.g32.cpu(), "n16": flat.n16, "nd": flat.nd}, out % rank)
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_table_gradient_before_the_optimiser_equals_single_process(N, O, dev, tmp_path):
    """The quantity the exchange carries, compared BEFORE AdamW's sign normalisation can hide its size: 2 ranks (both on
    cuda:0, gloo carrying the collectives) x 4096 rays each run their shard's HIP backward, reduce-scatter the loss-scaled
    fp16 table gradient and all-reduce the fp32 dense gradients exactly as FlatAdamW.step does; the single process runs the
    8192-ray batch.  Each rank's table gradient is the fp16 rounding of an exact fixed-point bin sum, the collective adds two
    of those in fp16: three roundings of 2^-11 against the single process's one.  Bounds (stated, measured into
    gpurun_out/r06_parity.json): the collective's own sum vs the exact fp64 sum of the two rank gradients rel-L2 <= 3e-4 (one
    fp16 rounding); reduced vs single-process table gradient rel-L2 <= 6e-4, no entry further off than 2^-10 of the largest
    gradient, and on the HASHED levels (binned exact sums, except the records of a bin segment that overflowed its 48 staging
    slots, which take the packed-fp16-atomic path -- and which records overflow depends on how many points a workgroup
    sees, i.e. on the shard size) every entry within 2^-7 (|g_0| + |g_1| + |g|) + one fp16 subnormal step (measured worst:
    4.7 x 2^-10).  The dense coarse levels accumulate with packed fp16 atomics throughout (tiny-cuda-nn's own mode: one
    rounding per add, in whatever order the points arrive), so there an entry's error scales with its partial sums, not
    its value: rel-L2 1.1e-3 measured, <= 3e-3 required; dense parameter gradients + loss rel 2e-4."""
    import json
    import torch.multiprocessing as mp
    from go_slam_amd.neus.mapper import MapTrainer
    out = str(tmp_path / "grad%d.pt")
    mp.start_processes(_one_gpu_rank_gradients, args=(2, 29500 + (os.getpid() % 400), out), nprocs=2, join=True,
                       start_method="spawn")
    r = [torch.load(out % k) for k in range(2)]
    n16, nd = r[0]["n16"], r[0]["nd"]
    assert r[0]["lo"] == 0 and r[0]["hi"] == r[1]["lo"] and r[1]["hi"] >= n16 and r[0]["inv_scale"] == r[1]["inv_scale"]
    reduced = torch.cat([r[0]["slice"], r[1]["slice"]])[:n16].double() * r[0]["inv_scale"]
    loc = [x["local"][:n16].double() * r[0]["inv_scale"] for x in r]
    exact = loc[0] + loc[1]
    assert bool(torch.isfinite(reduced).all()) and float((loc[0] != 0).double().mean()) > 0.01
    assert float(((loc[0] != 0) & (loc[1] != 0)).double().mean()) > 0.005, "the shards must meet in table entries"
    P = O.make_params(171, grid_init=0.05, bound=((-2.5, 2.5), (-2.5, 2.5), (-2.5, 2.5)))
    model = N.InstantNeuS({}, P["bound"].tolist()).to(dev)
    _load(model, P)
    tr = MapTrainer(model, N.Renderer(N_samples=24, N_surface=48))
    o, d, gt = _rays(8192, seed=172)
    g = torch.Generator().manual_seed(173)
    args = [t.to(dev) for t in (o, d, torch.rand(8192, 3, generator=g), gt, torch.rand(24, generator=g))]
    loss, g16, inv_scale = tr.fused_gradients(*args)
    assert inv_scale == r[0]["inv_scale"]
    single = g16.double().cpu() * inv_scale
    rel = lambda a, b: float((a - b).norm() / b.norm())
    sub = 2.0 ** -24 * inv_scale                                    # one fp16 subnormal step of the scaled gradient
    bound = 2.0 ** -10 * (loc[0].abs() + loc[1].abs() + single.abs()) + sub
    meta = O.grid_meta()
    hashed = torch.zeros(n16, dtype=torch.bool)
    for l in range(16):
        if int(meta["hashed"][l]):
            hashed[2 * int(meta["offset"][l]):2 * (int(meta["offset"][l]) + int(meta["size"][l]))] = True
    assert bool(hashed.any()) and not bool(hashed.all())
    worst = float(((reduced - single).abs() / bound)[hashed].max())
    worst_dense = float(((reduced - single).abs() / bound)[~hashed].max())
    rec = {"rays_per_rank": 4096, "table_entries_touched": int((single != 0).sum()),
           "collective_vs_exact_sum_rel_l2": rel(reduced, exact), "reduced_vs_single_rel_l2": rel(reduced, single),
           "exact_sum_vs_single_rel_l2": rel(exact, single), "max_abs_diff": float((reduced - single).abs().max()),
           "max_abs_grad": float(single.abs().max()), "worst_hashed_entry_over_bound": worst,
           "worst_dense_level_entry_over_bound": worst_dense,
           "dense_levels_rel_l2": rel(reduced[~hashed], single[~hashed]), "hashed_levels_rel_l2": rel(reduced[hashed], single[hashed]),
           "dense_rel_l2": rel(r[0]["g32"][:nd].double(), tr.flat.g32[:nd].double().cpu())}
    d_ = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")
    try:
        os.makedirs(d_, exist_ok=True)
        path = os.path.join(d_, "r06_parity.json")
        cur = json.load(open(path)) if os.path.exists(path) else {}
        cur["sharded_table_gradient_2_ranks_vs_single_process"] = rec
        json.dump(cur, open(path, "w"), indent=1, sort_keys=True)
    except OSError:
        pass
    assert rec["collective_vs_exact_sum_rel_l2"] <= 3e-4, rec
    assert rec["reduced_vs_single_rel_l2"] <= 6e-4, rec
    assert worst <= 8.0, rec
    assert rec["dense_levels_rel_l2"] <= 3e-3 and rec["hashed_levels_rel_l2"] <= 6e-4, rec
    assert rec["max_abs_diff"] <= 2.0 ** -10 * rec["max_abs_grad"], rec
    assert torch.equal(reduced != 0, single != 0) or float(((reduced != 0) != (single != 0)).double().mean()) < 1e-4
    torch.testing.assert_close(r[0]["g32"][:nd], tr.flat.g32[:nd].cpu(), rtol=2e-4, atol=1e-6)
    torch.testing.assert_close(r[0]["g32"][nd], loss.cpu(), rtol=2e-4, atol=1e-6)
    assert torch.equal(r[0]["g32"], r[1]["g32"])


def _rccl_world1(_index, port, out):
    """the sharded mapper step and bench.py's collective self-test in an RCCL process group of ONE rank"""
    import os
    import sys
    import torch.distributed as dist
    from go_slam_amd.neus.mapper import MapTrainer
    import go_slam_amd.neus as neus
    from oracle import neus_oracle as NO
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    res = {"backend": dist.get_backend()}
    try:
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        import bench
        res["selftest"] = bench.collectives_selftest(dev, 0, 1)
        P = NO.make_params(71, grid_init=0.05, bound=((-2.5, 2.5), (-2.5, 2.5), (-2.5, 2.5)))
        model = neus.InstantNeuS({}, P["bound"].tolist()).to(dev)
        _load(model, P)
        tr = MapTrainer(model, neus.Renderer(N_samples=24, N_surface=48), rank=0, world=1, sharded=True)
        o, d, gt = _rays(600, seed=72)
        g = torch.Generator().manual_seed(73)
        args = [t.to(dev) for t in (o, d, torch.rand(600, 3, generator=g), gt, torch.rand(24, generator=g))]
        for _ in range(5):              # 2 eager + capture (two graphs around the early reduce-scatter) + 2 replays
            loss = tr.step(*args)
        res["one_graph_now"] = tr._one_graph()
        with torch.no_grad():           # a render between steps waits for the deferred all-gather through the cache hook
            res["pending_before_render"] = tr.flat._gather_wait is not None
            model(args[0][:8], args[1][:8], *tr.renderer.sample(args[0][:8], args[1][:8], model.bound, args[3][:8]))
            res["pending_after_render"] = tr.flat._gather_wait is not None
        res.update(loss=float(loss), sd={k: v.detach().cpu() for k, v in tr.state_dict().items()},
                   graphs=len(tr._graphs), two_graphs=all(e.get("tail") is not None for e in tr._graphs.values()),
                   one_graph=all(bool(e.get("one")) for e in tr._graphs.values()),
                   capture_error=tr.capture_collectives_error)
        torch.cuda.synchronize()
    finally:
        dist.destroy_process_group()
    torch.save(res, out)


def test_sharded_schedule_runs_under_rccl_in_a_one_rank_group(N, O, dev, tmp_path):
    """What a 1-GPU box can say about the RCCL path: `MapTrainer(..., sharded=True)` runs the world > 1 schedule -- counts
    outside the graph, TWO hipGraphs captured around the early reduce-scatter (thread-local capture beside RCCL's
    watchdog thread), fp16 reduce-scatter, slice AdamW, deferred in-place fp16 all-gather waited for by the next reader
    -- in a `nccl` process group of one rank, where the collectives are RCCL's own one-rank copies on its own stream.
    Five steps must equal the plain single-process trainer; bench.py's collective self-test must pass on the same
    group.  (The exchange between GPUs itself stays unmeasured: tests/test_distributed_gpu.py needs two.)"""
    import torch.multiprocessing as mp
    from go_slam_amd.neus.mapper import MapTrainer
    out = str(tmp_path / "rccl1.pt")
    mp.start_processes(_rccl_world1, args=(29300 + (os.getpid() % 600), out), nprocs=1, join=True, start_method="spawn")
    got = torch.load(out)
    assert got["backend"] == "nccl" and got["selftest"] == (True, ""), got.get("selftest")
    # round 6: the step is ONE hipGraph with the RCCL enqueues captured in it (then nothing is deferred: the all-gather is a
    # node of the graph); where RCCL / torch refuse the capture, the reason is recorded and the round-5 schedule runs (two
    # graphs around eager collectives, the all-gather waited for by the table's next reader)
    assert got["graphs"] == 1
    if got["one_graph"]:
        assert got["capture_error"] is None and not got["two_graphs"] and not got["pending_before_render"]
    else:
        assert got["capture_error"] is not None and got["two_graphs"], got
        assert got["pending_before_render"] and not got["pending_after_render"]
    P = O.make_params(71, grid_init=0.05, bound=((-2.5, 2.5), (-2.5, 2.5), (-2.5, 2.5)))
    model = N.InstantNeuS({}, P["bound"].tolist()).to(dev)
    _load(model, P)
    tr = MapTrainer(model, N.Renderer(N_samples=24, N_surface=48))
    o, d, gt = _rays(600, seed=72)
    g = torch.Generator().manual_seed(73)
    args = [t.to(dev) for t in (o, d, torch.rand(600, 3, generator=g), gt, torch.rand(24, generator=g))]
    for _ in range(5):
        loss = tr.step(*args)
    assert abs(got["loss"] - float(loss)) < 3e-4 * max(1.0, abs(float(loss)))
    trained = {"sdf_network.encoding.encoding.params", "sdf_network.sdf_layer.weight", "sdf_network.sdf_layer.bias",
               "color_network._B", "color_network.network.params", "variance_network.variance"}
    for k, v in tr.state_dict().items():
        if k not in trained:
            continue
        a, b = got["sd"][k].float(), v.detach().cpu().float()
        dlt = (a - b).abs()
        lr = 1e-2 if k.endswith("encoding.params") else 1e-3
        off = dlt > (2e-5 + 2e-3 * b.abs())         # (as the two-rank test: a handful of +-lr flips of rounding-level gradients)
        assert float(off.float().mean()) < 1e-2 and float(dlt.max()) <= 5 * lr * 1.01, (k, float(off.float().mean()), float(dlt.max()))


def _grid_grads(N, O, dev, P, rays, binned, grad_dtype):
    model = N.InstantNeuS({}, P["bound"].tolist()).to(dev)
    _load(model, P)
    model.grid_grad_dtype = grad_dtype
    model.grid_grad_binned = binned
    o, d, z, dist = rays
    out = model(o.to(dev), d.to(dev), z.to(dev), dist.to(dev))
    loss = (out["color"].sum() + 0.3 * out["depth"].sum() + out["sdf"][out["sdf"] != 100.0].sum()) / o.shape[0] \
        + 0.1 * out["gradient_error"].sum()       # (a mean: the fp16 table gradient carries loss scale 128, max 65504)
    loss.backward()
    return model.sdf_network.encoding.encoding.params.grad.detach().float().cpu()


def test_binned_table_gradient_equals_atomic_accumulation(N, O, dev):
    """The hashed levels' table gradient by bin-and-reduce (no global atomics: per-bin record queues + exact 64-bit
    fixed-point LDS sums, csrc/neus_bwd.hip grid_bin_reduce_kernel) vs fp32 atomics on the same rays: equal to fp16
    record rounding -- and CLOSER to the fp32 result than tiny-cuda-nn's fp16 packed atomics are."""
    P = O.make_params(81, grid_init=0.3, bound=((-2.5, 2.5), (-2.5, 2.5), (-2.5, 2.5)))
    o, d, gt = _rays(3000, seed=82)
    g = torch.Generator().manual_seed(83)
    z, dist = O.render_sample(o, d, gt, P["bound"], 24, 48, torch.rand(24, generator=g))
    rays = (o, d, z, dist)
    ref = _grid_grads(N, O, dev, P, rays, False, torch.float32)
    binned = _grid_grads(N, O, dev, P, rays, True, torch.float16)
    atom16 = _grid_grads(N, O, dev, P, rays, False, torch.float16)
    gm = O.grid_meta()
    e_bin, e_atom = [], []
    for l in range(16):
        a, b = 2 * int(gm["offset"][l]), 2 * (int(gm["offset"][l]) + int(gm["size"][l]))
        e_bin.append(_rel(binned[a:b], ref[a:b]))
        e_atom.append(_rel(atom16[a:b], ref[a:b]))
    hashed = [l for l in range(16) if int(gm["hashed"][l])]
    assert len(hashed) == 11
    assert max(e_bin) < 2e-3, e_bin
    assert all(e_bin[l] <= e_atom[l] * 1.05 + 1e-6 for l in hashed), (e_bin, e_atom)
    assert max(e_bin[l] for l in hashed) < 3e-4, e_bin          # one fp16 rounding per record, fp32 sums


def test_binned_table_gradient_staging_overflow_falls_back_to_atomics(N, O, dev):
    """Adversarial input for the record staging: 512 one-sample rays alternating between TWO positions, so that every
    level receives all its records on 16 entries -- no run of equal cells for the wave to pre-reduce, and each
    workgroup's staging bins (48 slots) see 128 records per entry.  The excess must continue as packed atomics: nothing
    may be dropped.  (Kept small on purpose: an fp16 sum of n equal addends rounds at every step, with a bias that
    grows with n -- tiny-cuda-nn's own accumulation, which the all-atomics mode shows on the same input.)"""
    P = O.make_params(91, grid_init=0.3, bound=((-2.5, 2.5), (-2.5, 2.5), (-2.5, 2.5)))
    n = 512
    o = torch.zeros(n, 3)
    o[0::2] = torch.tensor([0.31, -0.42, 0.17])
    o[1::2] = torch.tensor([-1.13, 0.77, -0.58])
    d = torch.nn.functional.normalize(torch.tensor([[0.2, 0.5, -0.3]]), dim=1).repeat(n, 1)
    z = torch.full((n, 1), 0.05)
    dist = torch.full((n, 1), 0.02)
    rays = (o, d, z, dist)
    ref = _grid_grads(N, O, dev, P, rays, False, torch.float32)
    binned = _grid_grads(N, O, dev, P, rays, True, torch.float16)
    atom16 = _grid_grads(N, O, dev, P, rays, False, torch.float16)
    nz = ref.abs() > 1e-6 * ref.abs().max()
    assert 16 * 2 * 8 // 2 <= int(nz.sum()) <= 16 * 2 * 16         # two points x 8 corners x 2 features x 16 levels
    rel = ((binned - ref).abs() / ref.abs())[nz]
    # 256 records per entry: 96 summed exactly through the queues, 160 by fp16 atomics.  A dropped overflow path would
    # lose 60 % of every entry; fp16 accumulation alone (the all-atomics mode) explains a few per cent at most.
    assert float(rel.max()) < 6e-2 and _rel(binned, ref) < 2e-2, (float(rel.max()), _rel(binned, ref))
    assert _rel(binned, ref) <= 1.2 * _rel(atom16, ref) + 2e-3, (_rel(binned, ref), _rel(atom16, ref))
    # an ordinary batch right after gives the ordinary result (no state left behind)
    o2, d2, gt2 = _rays(500, seed=92)
    z2, dist2 = O.render_sample(o2, d2, gt2, P["bound"], 24, 48, None)
    a = _grid_grads(N, O, dev, P, (o2, d2, z2, dist2), True, torch.float16)
    b = _grid_grads(N, O, dev, P, (o2, d2, z2, dist2), False, torch.float32)
    assert _rel(a, b) < 2e-3


def test_graph_replay_follows_update_bound_and_survives_buffer_eviction(N, O, dev):
    """Two defects a captured step must not have (round-3 advisor findings).  (1) `InstantNeuS.update_bound` between
    replays: the realtime bound is read from the model's device buffer, so the replay masks with the CURRENT bound
    (src/InstantNeuS.py:310) exactly as the eager step does -- a bound passed by value would be frozen at capture time
    and the two trainers would part ways after the change.  (2) The per-batch-size step buffers a graph points into are
    owned by the graph entry: running more distinct batch sizes than the buffer cache holds must not free them."""
    from go_slam_amd.neus import mapper as M
    P = O.make_params(101, grid_init=0.05, bound=((-2.5, 2.5), (-2.5, 2.5), (-2.5, 2.5)))
    trainers = []
    for graph in (False, True):
        model = N.InstantNeuS({}, P["bound"].tolist()).to(dev)
        _load(model, P)
        trainers.append((model, M.MapTrainer(model, N.Renderer(N_samples=24, N_surface=48), graph=graph)))
    (m_e, t_e), (m_g, t_g) = trainers
    g = torch.Generator().manual_seed(102)
    small = torch.tensor([[-0.6, 0.7], [-0.8, 0.5], [-0.4, 0.9]])
    big = torch.tensor([[-2.5, 2.5], [-2.5, 2.5], [-2.5, 2.5]])
    for m in (m_e, m_g):
        m.update_bound(small)

    def both(it, n=640):
        o, d, gt = _rays(n, seed=200 + it)
        args = [t.to(dev) for t in (o, d, torch.rand(n, 3, generator=g), gt, torch.rand(24, generator=g))]
        l_e, l_g = t_e.step(*args), t_g.step(*args)
        torch.testing.assert_close(l_g.float().cpu(), l_e.float().cpu(), rtol=3e-4, atol=1e-5,
                                   msg=lambda s: f"iteration {it}: {s}")
        return float(l_e)
    for it in range(4):                         # two eager warm-ups, capture, replay -- all under the small bound
        both(it)
    ent = next(iter(t_g._graphs.values()))
    assert ent["graph"] is not None
    l_small = both(4)
    for m in (m_e, m_g):
        m.update_bound(big)                     # the scene grew (multiview_filter -> Mapper.__call__ -> update_bound)
    l_big = both(5)                             # a REPLAY of the graph captured under the small bound
    assert abs(l_big - l_small) > 1e-3 * abs(l_small), "the bound change did not alter the loss: test is vacuous"
    both(6)
    # (2) more batch sizes than the buffer cache keeps; then the first graph again
    owned = ent["bufs"]["counts"].data_ptr()
    o, d, gt = _rays(64, seed=400)
    for k in range(2 * M.MAX_GRAPHS + 2):
        n = 32 + k
        t_g._step_buffers(n, dev)
    assert 640 not in t_g._bufs                 # evicted from the cache ...
    assert ent["bufs"]["counts"].data_ptr() == owned        # ... but alive in the entry
    junk = [torch.full((3,), float("nan"), device=dev) for _ in range(64)]   # would land in freed 12-byte blocks
    both(7)
    both(8)
    del junk


def test_graph_cache_evicts_least_recently_used(N, O, dev):
    """more (shape, learning-rate) combinations than MAX_GRAPHS: the least recently used graph is dropped and the new
    combination is captured -- the step never degrades to the eager ~65-launch path for good."""
    from go_slam_amd.neus import mapper as M
    P = O.make_params(111, grid_init=0.05, bound=((-2.5, 2.5), (-2.5, 2.5), (-2.5, 2.5)))
    model = N.InstantNeuS({}, P["bound"].tolist()).to(dev)
    _load(model, P)
    tr = M.MapTrainer(model, N.Renderer(N_samples=24, N_surface=48))
    o, d, gt = _rays(128, seed=112)
    args = [t.to(dev) for t in (o, d, torch.rand(128, 3), gt)]
    for k in range(M.MAX_GRAPHS + 2):
        tr.optimizer.set_lr(grid_lr=1e-2 * (1 + k))
        for _ in range(3):
            loss = tr.step(*args)
        assert torch.isfinite(loss)
    assert len(tr._graphs) == M.MAX_GRAPHS
    keys = list(tr._graphs)
    assert keys[-1][3] == 1e-2 * (M.MAX_GRAPHS + 2) and all(k[3] != 1e-2 for k in keys)     # the oldest lr is gone
    assert tr._graphs[keys[-1]]["graph"] is not None


def test_binned_table_gradient_keeps_non_finite_records_visible(N, O, dev):
    """A diverged step must stay visible: with a NaN upstream gradient on ONE ray, the table entries that ray touches are
    non-finite in the binned mode exactly as with tiny-cuda-nn's packed atomics (the bin reduce's fixed-point sums
    saturate NaN / inf records, so it re-scans a bin that saw one and writes those records' own bits), and every other
    entry is the ordinary finite sum."""
    P = O.make_params(121, grid_init=0.3, bound=((-2.5, 2.5), (-2.5, 2.5), (-2.5, 2.5)))
    o, d, gt = _rays(300, seed=122)
    z, dist = O.render_sample(o, d, gt, P["bound"], 24, 48, None)
    res = {}
    for binned in (True, False):
        model = N.InstantNeuS({}, P["bound"].tolist()).to(dev)
        _load(model, P)
        model.grid_grad_dtype, model.grid_grad_binned = torch.float16, binned
        out = model(o.to(dev), d.to(dev), z.to(dev), dist.to(dev))
        poison = torch.zeros(300, 3, device=dev)
        poison[7] = float("nan")
        loss = (out["color"].sum() + 0.3 * out["depth"].sum()) / 300 + (out["color"] * poison)[7].sum()
        loss.backward()
        res[binned] = model.sdf_network.encoding.encoding.params.grad.detach().float().cpu()
    gm = O.grid_meta()
    bad_b, bad_a = ~torch.isfinite(res[True]), ~torch.isfinite(res[False])
    lo = 2 * int(gm["offset"][5])                  # first hashed level
    assert int(gm["hashed"][5]) and not int(gm["hashed"][4])
    assert int(bad_a[lo:].sum()) > 100, "the poisoned ray left no trace in the atomics mode: test is vacuous"
    assert torch.equal(bad_b, bad_a), (int(bad_b.sum()), int(bad_a.sum()))
    ok = ~bad_a
    assert _rel(res[True][ok], res[False][ok]) < 5e-3


@pytest.mark.parametrize("with_depth", [True, False])
def test_render_rays_equals_render_batch_ray_and_the_oracle_at_4096_rays(N, O, dev, with_depth):
    """`InstantNeuS.render_rays(rays_o, rays_d, gt_depth)` -- the entry point BASELINE.json's north_star names -- against
    (i) `Renderer.render_batch_ray(rays_o, rays_d, net, None, device, gt_depth)` (src/render.py:73-175) under the same device
    generator state: bit for bit, every one of the 9 outputs; (ii) the oracle's restatement of render.py:99-171 +
    InstantNeuS.py:295-370 with the `torch.rand(N_samples)` vector the call drew: sample positions bit-exact, the rest at
    the tolerances of test_neus_forward_matches_oracle.  4096 rays x 72 (24 + 48) samples with depth, x 24 without."""
    P = O.make_params(17, grid_init=0.3, bound=((-2.5, 2.5), (-2.5, 2.5), (-2.5, 2.5)))
    P["rt_bound"] = torch.tensor([[-2.2, 2.3], [-2.4, 2.1], [-2.0, 2.2]])
    o, d, gt = _rays(4096, seed=18)
    gt = gt if with_depth else None
    model = N.InstantNeuS({}, P["bound"].tolist()).to(dev)
    _load(model, P)
    model.update_bound(P["rt_bound"])
    od, dd, gd = o.to(dev), d.to(dev), (gt.to(dev) if with_depth else None)
    with torch.no_grad():
        torch.manual_seed(1234)
        a = model.render_rays(od, dd, gd)
        torch.manual_seed(1234)
        b = N.Renderer(N_samples=24, N_surface=48).render_batch_ray(od, dd, model, None, dev, gd)
        torch.manual_seed(1234)
        pr = torch.rand(24, device=dev).cpu()                      # the reference's draw (render.py:159)
        c = model.render_rays(od, dd, gd)                           # a second call continues the generator stream
    assert set(a) == set(b) == {"color", "depth", "depth_variance", "normal", "weight_sum", "sdf_variance", "sdf", "z_vals",
                                "gradient_error"}
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert not torch.equal(a["z_vals"], c["z_vals"]), "every batch draws a new perturbation vector"
    z, dist = O.render_sample(o, d, gt, P["bound"], 24, 48, pr)
    ref = O.neus_forward(o, d, z, dist, P)
    got = {k: v.cpu() for k, v in a.items()}
    assert tuple(got["sdf"].shape) == (4096, 72 if with_depth else 24)
    assert torch.equal(got["z_vals"], ref["z_vals"])
    assert torch.equal(got["sdf"] == 100.0, ref["sdf"] == 100.0)
    torch.testing.assert_close(got["sdf"], ref["sdf"], rtol=1e-4, atol=2e-5)
    torch.testing.assert_close(got["weight_sum"], ref["weight_sum"], rtol=0, atol=5e-4)
    torch.testing.assert_close(got["depth"], ref["depth"], rtol=0, atol=2e-3)
    torch.testing.assert_close(got["depth_variance"], ref["depth_variance"], rtol=1e-2, atol=2e-3)
    torch.testing.assert_close(got["color"], ref["color"], rtol=0, atol=4e-3)
    torch.testing.assert_close(got["normal"], ref["normal"], rtol=2e-3, atol=2e-3)
    torch.testing.assert_close(got["gradient_error"], ref["gradient_error"], rtol=2e-3, atol=1e-5)
    torch.testing.assert_close(got["sdf_variance"], ref["sdf_variance"])


def test_renderer_consumes_the_device_generator_like_the_reference(N, dev):
    """render.py:159 draws `torch.rand(N_samples, device=device)` once per batch; the default Renderer issues that very call,
    so under a seed the k-th batch gets the k-th such draw and the generator is left where the reference leaves it (the
    mapper's `randint` pixel draws in between see the same stream).  `rand_pool_rows > 1` trades that for one launch per
    `rows` batches and is NOT stream-compatible (checked: it must differ, or the flag documents nothing)."""
    R = N.Renderer(N_samples=24, N_surface=48)
    torch.manual_seed(77)
    rows = [R._perturb_row(24, dev).clone() for _ in range(3)]
    after = torch.randint(0, 1 << 30, (4,), device=dev)
    torch.manual_seed(77)
    ref = [torch.rand(24, device=dev) for _ in range(3)]
    ref_after = torch.randint(0, 1 << 30, (4,), device=dev)
    assert all(torch.equal(a, b) for a, b in zip(rows, ref)) and torch.equal(after, ref_after)
    Rp = N.Renderer(N_samples=24, N_surface=48, rand_pool_rows=128)
    torch.manual_seed(77)
    pooled = [Rp._perturb_row(24, dev).clone() for _ in range(3)]
    assert not all(torch.equal(a, b) for a, b in zip(pooled, ref))
    assert float(torch.stack(pooled).min()) >= 0.0 and float(torch.stack(pooled).max()) < 1.0


@pytest.mark.parametrize("H,W,F,n_rays", [(24, 40, 5, 37), (480, 640, 20, 220)])
def test_ray_bank_device_draw_equals_build_rays(N, dev, H, W, F, n_rays):
    """neus/rays.RayBank on the device (the reference's randint calls + ONE gs_ray_draw launch) against build_rays called
    frame by frame on the device (src/nerf_func.py:115-181, src/mapping.py:222-240) under the same seed: the same pixels --
    origins, colours, depths bit for bit, directions to fp32 rounding of the 3 x 3 product -- with ragged masks, a frame
    without a mask, repeated frames, a numpy pose; and the same generator consumption (the next draw after either is
    the same)."""
    import numpy as np
    from go_slam_amd.neus import rays as R
    g = torch.Generator().manual_seed(5)
    fx, fy, cx, cy = 0.9 * W, 0.91 * W, W / 2 - 0.5, H / 2 - 0.5
    items = {}
    for f in range(F):
        c2w = torch.eye(4)
        q = torch.linalg.qr(torch.randn(3, 3, generator=g))[0]
        c2w[:3, :3], c2w[:3, 3] = q, torch.randn(3, generator=g)
        mask = (torch.rand(H, W, generator=g) < (0.3 + 0.6 * f / F)).float().to(dev) if f != 2 else None
        items[10 + f] = (torch.rand(H, W, 3, generator=g).to(dev), (torch.rand(H, W, generator=g) * 3 + 0.5).to(dev),
                         c2w.numpy() if f == 1 else c2w.to(dev), None, mask)
    bank = R.RayBank(items, H, W, fx, fy, cx, cy, dev)
    assert bank.fused
    assert bank.N[2] == H * W and all(0 < n <= H * W for n in bank.N)
    frames = [10 + k for k in (2, 0, F - 1, 0, 3)] + [10 + k for k in range(F)]

    def per_frame():
        parts = [[], [], [], []]
        for f in frames:
            color, depth, c2w, _, mask = items[f]
            out = R.build_rays(0, H, 0, W, n_rays, H, W, fx, fy, cx, cy, c2w, depth, color, dev,
                               nerf_coordinate=False, dir_normalize=False, mask=mask)
            for acc, x in zip(parts, out):
                acc.append(x.float())
        o, d, dep, col = (torch.cat(p, 0) for p in parts)
        return o, d, col, dep
    torch.manual_seed(77)
    want = per_frame()
    nxt = torch.rand(3, device=dev)
    torch.manual_seed(77)
    got = bank.sample(frames, n_rays)
    assert torch.equal(torch.rand(3, device=dev), nxt)
    assert got[0].shape == (n_rays * len(frames), 3)
    assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[2]) and torch.equal(got[3], want[3])
    torch.testing.assert_close(got[1], want[1], rtol=1e-6, atol=1e-6)
    # the first and the last valid pixel of a frame (ranks 0 and N - 1) land where nonzero puts them
    p = bank.pos[10]
    first_last = torch.tensor([[0] * n_rays, [bank.N[p] - 1] * n_rays], dtype=torch.int64, device=dev)
    keep = torch.nonzero(items[10][4].reshape(-1).bool()).reshape(-1)
    import go_slam_amd._lib as _lib
    f32 = dict(dtype=torch.float32, device=dev)
    o, d, c = (torch.empty(2 * n_rays, 3, **f32) for _ in range(3))
    z = torch.empty(2 * n_rays, **f32)
    fp = torch.tensor([p, p], dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().gs_ray_draw(_lib.ptr(first_last), _lib.ptr(fp), _lib.ptr(bank.cum32), _lib.ptr(bank.color),
                                      _lib.ptr(bank.depth), _lib.ptr(bank.rot_t), _lib.ptr(bank.trans), 2, n_rays, H * W, W,
                                      fx, fy, cx, cy, _lib.ptr(o), _lib.ptr(d), _lib.ptr(c), _lib.ptr(z),
                                      _lib.stream_ptr(dev)), "ray_draw")
    depth10 = items[10][1].reshape(-1)
    assert torch.equal(z[:n_rays], depth10[keep[0]].expand(n_rays)) and torch.equal(z[n_rays:], depth10[keep[-1]].expand(n_rays))


@pytest.mark.parametrize("n", [1, 5, 257, 4096, 4099])
def test_render_sample_in_launch_batch_maximum_equals_the_reduction_launch(N, dev, n):
    """Renderer.sample with the batch's depth maximum taken inside the sampling launch (gs_render_sample with gt_max = -inf)
    against the same call fed `gt_depth.max()` as a device scalar (src/render.py:121,140): bit for bit, at sizes that end
    inside a 16-byte piece and inside a 1024-thread stride, with depth-less rays, with all depths zero, and with a NaN
    depth (torch.max propagates it: so must the launch)."""
    o, d, gt = _rays(n, seed=11)
    R = N.Renderer(N_samples=24, N_surface=48)
    bound = torch.tensor([[-5.0, 5.0], [-4.0, 4.5], [-3.0, 6.0]], device=dev)
    g = torch.Generator().manual_seed(2)
    pr = torch.rand(24, generator=g).to(dev)
    cases = [gt.clone(), torch.zeros(n)]
    bad = gt.clone()
    bad[n // 2] = float("nan")
    cases.append(bad)
    for k, depth in enumerate(cases):
        depth = depth.to(dev)
        z1, d1 = R.sample(o.to(dev), d.to(dev), bound, depth, pr)                                  # in-launch maximum
        z2, d2 = R.sample(o.to(dev), d.to(dev), bound, depth, pr, gt_max_dev=depth.max().reshape(1))
        if k == 2:      # a NaN maximum: the far bound and the depth-less rays' samples are NaN in both forms (the merge's
            assert bool(z1.isnan().any()) and bool(z2.isnan().any())       # ranks are then undefined: no slot-wise claim)
            continue
        assert not bool(z1.isnan().any()) and torch.equal(z1, z2) and torch.equal(d1, d2)
