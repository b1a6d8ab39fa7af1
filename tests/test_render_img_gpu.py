"""Renderer.render_img and the image metrics on the MI355X: against the reference's own render_img / Visualizer.vis
(tests/golden/render_img.npz), against per-batch gs_render_sample and per-piece gs_neus_forward calls, against the
batch loop of render_batch_ray + cat at full frame sizes, and against fp64 torch."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = ("color", "depth", "depth_variance", "normal", "weight_sum", "sdf_variance", "sdf", "z_vals", "gradient_error")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def N(built_lib):
    import go_slam_amd.neus as neus
    return neus


@pytest.fixture(scope="module")
def G():
    return {k: np.asarray(v) for k, v in np.load(os.path.join(HERE, "golden", "render_img.npz")).items()}


def _model(N, dev, seed, bound, rt_bound=None):
    from oracle import neus_oracle as NO
    P = NO.make_params(seed, grid_init=0.3, bound=tuple(tuple(float(x) for x in r) for r in bound))
    model = N.InstantNeuS({}, P["bound"].tolist()).to(dev)
    with torch.no_grad():
        model.sdf_network.encoding.encoding.params.copy_(P["grid"])
        model.sdf_network.sdf_layer.weight.copy_(P["sdf_w"])
        model.sdf_network.sdf_layer.bias.copy_(P["sdf_b"])
        model.color_network._B.copy_(P["color_B"])
        model.color_network.network.params.copy_(P["mlp"])
        model.variance_network.variance.fill_(P["variance"])
    if rt_bound is not None:
        model.update_bound(torch.as_tensor(rt_bound, dtype=torch.float32))
        P["rt_bound"] = torch.as_tensor(rt_bound, dtype=torch.float32)
    return model, P


def _renderer(N, G, tag=None, **kw):
    cam = {k: float(G[k]) for k in ("fx", "fy", "cx", "cy")}
    if tag is not None:
        kw.update(ray_batch_size=int(G[f"ray_batch_{tag}"]), points_batch_size=int(G[f"points_batch_{tag}"]))
    return N.Renderer(N_samples=24, N_surface=48, H=int(G["H"]), W=int(G["W"]), **cam, **kw)


def _rows_from(R, rows):
    it = iter(rows)
    R._perturb_row = lambda ns, device: next(it).to(device)


def _compare(out, ref, max_flips=4, tol=1.0, skip=None):
    """the forward's fixture tolerances (tests/test_neus_gpu.py), scaled by `tol`; rays whose in-bound mask differs in
    a point are left out (at most `max_flips` points), and so are the rays in `skip` (directions one rounding apart from
    the reference's: a sample that moves by an ulp can move a weight by 1e-3)"""
    o = {k: v.detach().float().cpu() for k, v in out.items()}
    r = {k: torch.as_tensor(v).float().cpu() for k, v in ref.items()}
    flip = (o["sdf"] == 100.0) != (r["sdf"] == 100.0)
    assert int(flip.sum()) <= max_flips, int(flip.sum())
    keep = ~flip.any(1)
    if skip is not None:
        assert float(skip.float().mean()) < 0.02
        keep &= ~skip
    skipped = not bool(keep.all())
    torch.testing.assert_close(o["z_vals"][keep], r["z_vals"][keep], rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(o["sdf"][keep], r["sdf"][keep], rtol=1e-4 * tol, atol=2e-5 * tol)
    torch.testing.assert_close(o["weight_sum"][keep], r["weight_sum"][keep], rtol=0, atol=5e-4 * tol)
    torch.testing.assert_close(o["depth"][keep], r["depth"][keep], rtol=0, atol=2e-3 * tol)
    torch.testing.assert_close(o["depth_variance"][keep], r["depth_variance"][keep], rtol=1e-2 * tol, atol=2e-3 * tol)
    torch.testing.assert_close(o["color"][keep], r["color"][keep], rtol=0, atol=4e-3 * tol)
    torch.testing.assert_close(o["normal"][keep], r["normal"][keep], rtol=2e-3 * tol, atol=2e-3 * tol)
    torch.testing.assert_close(o["sdf_variance"], r["sdf_variance"])
    assert o["gradient_error"].shape == r["gradient_error"].shape
    if not skipped:
        torch.testing.assert_close(o["gradient_error"], r["gradient_error"], rtol=2e-3 * tol, atol=1e-5 * tol)


# 1 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["a", "b"])
def test_render_img_matches_the_reference_fixture(N, G, dev, tag):
    model, _ = _model(N, dev, int(G["seed"]), G["bound"], G["rt_bound"])
    R = _renderer(N, G, tag)
    rows = torch.from_numpy(G[f"perturb_{tag}"])
    _rows_from(R, rows)
    gt = torch.from_numpy(G["gt_depth"]).to(dev)
    out = R.render_img(model, G["c2w"], dev, gt_depth=gt)
    _, rd, _, _, _ = R.image_samples(G["c2w"], model.bound, dev, gt, perturb_rows=rows.to(dev))
    erd = torch.from_numpy(G["rays_d"])
    assert set(out) == set(KEYS)
    H, W = int(G["H"]), int(G["W"])
    assert out["color"].shape == (H * W, 3) and out["depth"].shape == (H * W, 1) and out["sdf"].shape == (H * W, 72)
    assert out["gradient_error"].shape == G[f"gradient_error_{tag}"].shape
    _compare(out, {k: G[f"{k}_{tag}"] for k in KEYS}, skip=(rd.cpu() != erd).any(1))


def test_metrics_match_the_reference_visualizer(N, G, dev):
    from go_slam_amd.neus.image_vis import image_metrics
    ro = {k: torch.from_numpy(G[f"{k}_a"]).to(dev) for k in KEYS}
    imgs, m = image_metrics(ro, torch.from_numpy(G["gt_depth"]), torch.from_numpy(G["gt_color"]), G["c2w"])
    m = m.cpu().numpy()
    for i, k in enumerate(("mse", "psnr", "mae", "rmse", "s001", "s002")):
        np.testing.assert_allclose(m[i], float(G[f"metric_{k}"]), rtol=1e-5, err_msg=k)
    torch.testing.assert_close(imgs["normal_cam"].cpu(), torch.from_numpy(G["normal_cam"]), rtol=1e-5, atol=1e-6)
    assert torch.equal(imgs["depth_res"].cpu().reshape(-1), torch.from_numpy(G["depth_res"]).reshape(-1))
    assert torch.equal(imgs["color_res"].cpu().reshape(-1), torch.from_numpy(G["color_res"]).reshape(-1))


# 2 ------------------------------------------------------------------------------------------------------------------
def _frame(H, W, seed, zero_every=13):
    g = torch.Generator().manual_seed(seed)
    c2w = torch.eye(4)
    c2w[:3, :3] = torch.linalg.qr(torch.randn(3, 3, generator=g))[0]
    c2w[:3, 3] = torch.randn(3, generator=g) * 0.3
    depth = torch.rand(H * W, generator=g) * 3.5 + 0.5
    depth[::zero_every] = 0.0
    color = torch.rand(H * W, 3, generator=g)
    return c2w, depth, color


def test_image_rays_and_samples_equal_per_batch_render_sample(N, dev):
    import render_img_restatement as RR
    H, W, B = 37, 53, 700                              # 1961 rays: 2 full batches and a ragged one
    c2w, depth, _ = _frame(H, W, 31)
    depth[700:1400] = 0.0                              # a batch without depth (its maximum is 0)
    R = N.Renderer(N_samples=24, N_surface=48, ray_batch_size=B, H=H, W=W, fx=41.0, fy=42.5, cx=26.0, cy=18.5)
    bound = torch.tensor([[-5.0, 5.0], [-4.0, 4.5], [-3.0, 6.0]])
    g = torch.Generator().manual_seed(3)
    rows = torch.rand(3, 24, generator=g).to(dev)
    gt = depth.to(dev)
    ro, rd, z, d, gmax = R.image_samples(c2w, bound, dev, gt, perturb_rows=rows)
    ero, erd = RR.image_rays(H, W, 41.0, 42.5, 26.0, 18.5, c2w)
    torch.testing.assert_close(ro.cpu(), ero, rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(rd.cpu(), erd, rtol=1e-6, atol=1e-6)
    for b in range(3):
        sl = slice(b * B, min(H * W, (b + 1) * B))
        assert float(gmax[b]) == float(gt[sl].max())
        zb, db = R.sample(ro[sl], rd[sl], bound, gt[sl], perturb_rand=rows[b], gt_max_dev=gmax[b:b + 1])
        assert torch.equal(z[sl], zb) and torch.equal(d[sl], db), b
    # a NaN depth poisons its own batch's maximum only
    gt_nan = gt.clone()
    gt_nan[750] = float("nan")
    _, _, zn, dn, gmn = R.image_samples(c2w, bound, dev, gt_nan, perturb_rows=rows)
    assert torch.isnan(gmn[1]) and torch.equal(gmn[[0, 2]], gmax[[0, 2]])
    for sl in (slice(0, B), slice(2 * B, H * W)):
        assert torch.equal(zn[sl], z[sl]) and torch.equal(dn[sl], d[sl])
    # no depth image: render_batch_ray's no-depth branch, per batch
    ro0, rd0, z0, d0, gm0 = R.image_samples(c2w, bound, dev, None, perturb_rows=rows)
    assert gm0 is None and z0.shape == (H * W, 24)
    for b in range(3):
        sl = slice(b * B, min(H * W, (b + 1) * B))
        zb, db = R.sample(ro0[sl], rd0[sl], bound, None, perturb_rand=rows[b])
        assert torch.equal(z0[sl], zb) and torch.equal(d0[sl], db)


def test_render_img_without_depth(N, G, dev):
    model, _ = _model(N, dev, int(G["seed"]), G["bound"], G["rt_bound"])
    R = _renderer(N, G, "a")
    out = R.render_img(model, torch.from_numpy(G["c2w"]), dev)
    assert out["sdf"].shape == (int(G["H"]) * int(G["W"]), 24) and out["gradient_error"].numel() == 10
    assert all(bool(torch.isfinite(out[k]).all()) for k in KEYS)


# 3 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level_major", [False, True])
def test_segmented_forward_equals_per_piece_forward_calls(N, G, dev, level_major):
    from go_slam_amd import _lib
    from go_slam_amd.neus.instant_neus import _neus_forward_segmented_raw
    model, _ = _model(N, dev, int(G["seed"]), G["bound"], G["rt_bound"])
    R = _renderer(N, G, "a")
    g = torch.Generator().manual_seed(5)
    ro, rd, z, d, _ = R.image_samples(G["c2w"], model.bound, dev, torch.from_numpy(G["gt_depth"]).to(dev),
                                      perturb_rows=torch.rand(4, 24, generator=g).to(dev))
    n, s = z.shape
    L = _lib.lib()
    old = L.gs_neus_level_major_min_points(0 if level_major else 1 << 30)
    try:
        for B, P in ((300, 37), (300, 300), (256, 100), (960, 960)):     # 37 x 72 points: not a multiple of 64
            k = L.gs_neus_forward_pieces(n, B, P)
            f32 = dict(dtype=torch.float32, device=dev)
            out = {"color": torch.empty(n, 3, **f32), "depth": torch.empty(n, 1, **f32),
                   "depth_variance": torch.empty(n, 1, **f32), "normal": torch.empty(n, 3, **f32),
                   "weight_sum": torch.empty(n, 1, **f32), "sdf_variance": torch.empty(n, 1, **f32),
                   "sdf": torch.empty(n, s, **f32), "z_vals": torch.empty(n, s, **f32),
                   "gerr_ray": torch.empty(n, **f32), "gradient_error": torch.empty(k, **f32)}
            _neus_forward_segmented_raw(model, ro, rd, z, d, B, P, out)
            ref, forced = {}, 0
            with torch.no_grad():
                for b0 in range(0, n, B):
                    for p0 in range(b0, min(n, b0 + B), P):
                        p1 = min(p0 + P, b0 + B, n)
                        o = model(ro[p0:p1], rd[p0:p1], z[p0:p1], d[p0:p1])
                        forced += int((o["sdf"] != 100).sum()) == min(100, (p1 - p0) * s)
                        for key, v in o.items():
                            ref.setdefault(key, []).append(v)
            ref = {key: torch.cat(v) for key, v in ref.items()}
            assert len(ref["gradient_error"]) == k
            for key in KEYS[:-1]:
                assert torch.equal(out[key], ref[key]), (B, P, key)
            torch.testing.assert_close(out["gradient_error"], ref["gradient_error"], rtol=1e-6, atol=1e-9)
            if B == 300 and P == 37:
                assert forced > 0          # empty pieces between non-empty ones
    finally:
        L.gs_neus_level_major_min_points(old)


# 4 ------------------------------------------------------------------------------------------------------------------
def _batch_loop(R, model, ro, rd, gt, dev):
    out = {}
    for r0 in range(0, ro.shape[0], R.ray_batch_size):
        sl = slice(r0, r0 + R.ray_batch_size)
        o = R.render_batch_ray(ro[sl], rd[sl], model, device=dev, gt_depth=gt[sl])
        for k, v in o.items():
            out[k] = torch.cat([out[k], v]) if k in out else v
    return out


@pytest.mark.parametrize("H,W", [(480, 640), (680, 1200)])
def test_render_img_equals_the_batch_loop(N, dev, H, W):
    model, _ = _model(N, dev, 233, ((-4.0, 4.0), (-4.0, 4.0), (-4.0, 4.0)))
    c2w, depth, _ = _frame(H, W, 37)
    R = N.Renderer(N_samples=24, N_surface=48, H=H, W=W, fx=0.9 * W, fy=0.9 * W, cx=W / 2 - 0.5, cy=H / 2 - 0.5)
    gt = depth.to(dev)
    torch.manual_seed(11)
    out = R.render_img(model, c2w, dev, gt_depth=gt)
    torch.manual_seed(11)
    nb = -(-H * W // R.ray_batch_size)
    rows = torch.stack([torch.rand(24, device=dev) for _ in range(nb)])
    ro, rd, z, _, _ = R.image_samples(c2w, model.bound, dev, gt, perturb_rows=rows)
    assert torch.equal(out["z_vals"], _batch_loop_z(R, model, ro, rd, gt, rows))
    torch.manual_seed(11)
    ref = _batch_loop(R, model, ro, rd, gt, dev)
    assert torch.equal(out["sdf"] == 100.0, ref["sdf"] == 100.0)
    assert torch.equal(out["sdf"], ref["sdf"])                  # sdf: the same in either gather order
    _compare(out, ref, max_flips=0, tol=0.25)
    torch.testing.assert_close(out["gradient_error"], ref["gradient_error"], rtol=1e-4, atol=1e-7)


def _batch_loop_z(R, model, ro, rd, gt, rows):
    zs = []
    for b, r0 in enumerate(range(0, ro.shape[0], R.ray_batch_size)):
        sl = slice(r0, r0 + R.ray_batch_size)
        z, d = R.sample(ro[sl], rd[sl], model.bound, gt[sl], perturb_rand=rows[b])
        zs.append(z + d / 2.0)
    return torch.cat(zs)


def test_render_img_equals_the_restatement_mid_size(N, dev):
    import render_img_restatement as RR
    H, W, B, P = 60, 80, 1000, 384
    model, Pm = _model(N, dev, 239, ((-4.0, 4.0), (-4.0, 4.0), (-4.0, 4.0)), ((-3.0, 3.5), (-3.2, 3.0), (-2.9, 3.3)))
    c2w, depth, _ = _frame(H, W, 41)
    R = N.Renderer(N_samples=24, N_surface=48, ray_batch_size=B, points_batch_size=P, H=H, W=W, fx=70.0, fy=71.0,
                   cx=39.5, cy=29.5)
    rows = torch.rand(5, 24, generator=torch.Generator().manual_seed(9))
    _rows_from(R, rows)
    out = R.render_img(model, c2w, dev, gt_depth=depth.reshape(H, W).to(dev))
    _, rd, _, _, _ = R.image_samples(c2w, model.bound, dev, depth.to(dev), perturb_rows=rows.to(dev))
    ref = RR.render_img(Pm, H, W, 70.0, 71.0, 39.5, 29.5, c2w, depth, rows, B, P)
    _, erd = RR.image_rays(H, W, 70.0, 71.0, 39.5, 29.5, c2w)
    _compare(out, {k: ref[k] for k in KEYS}, max_flips=8, skip=(rd.cpu() != erd).any(1))


# 5 ------------------------------------------------------------------------------------------------------------------
def test_render_img_consumes_the_device_generator_like_the_reference(N, G, dev):
    model, _ = _model(N, dev, int(G["seed"]), G["bound"], G["rt_bound"])
    R = _renderer(N, G, "a")
    nb = -(-int(G["H"]) * int(G["W"]) // R.ray_batch_size)
    torch.manual_seed(77)
    R.render_img(model, G["c2w"], dev, gt_depth=torch.from_numpy(G["gt_depth"]).to(dev))
    after = torch.randint(0, 1 << 30, (4,), device=dev)
    torch.manual_seed(77)
    for _ in range(nb):
        torch.rand(24, device=dev)
    assert torch.equal(after, torch.randint(0, 1 << 30, (4,), device=dev))


# 6 ------------------------------------------------------------------------------------------------------------------
def test_metrics_kernel_against_fp64_torch(N, dev):
    from go_slam_amd.neus.image_vis import image_metrics
    n, s = 123457, 72
    g = torch.Generator().manual_seed(17)
    gt = torch.rand(n, generator=g) * 4
    gt[::7] = 0.0
    gt[3] = 1e-3
    ro = {"color": torch.rand(n, 3, generator=g), "depth": torch.rand(n, 1, generator=g) * 4,
          "normal": torch.randn(n, 3, generator=g), "sdf": torch.randn(n, s, generator=g) * 0.05}
    gc = torch.rand(n, 3, generator=g)
    c2w, _, _ = _frame(2, 2, 43)
    rod = {k: v.to(dev) for k, v in ro.items()}
    imgs, m = image_metrics(rod, gt.to(dev), gc.to(dev), c2w)
    imgs2, m2 = image_metrics(rod, gt.to(dev), gc.to(dev), c2w)
    assert torch.equal(m, m2) and all(torch.equal(imgs[k], imgs2[k]) for k in imgs)
    sel = gt > 1e-3
    de = (gt.double() - ro["depth"].reshape(-1).double()).abs()[sel]
    ce = (gc.double() - ro["color"].double())[sel]
    mse = (ce ** 2).mean()
    want = [mse, -10 * torch.log10(mse), de.mean(), (de ** 2).mean().sqrt(),
            (ro["sdf"].abs() < 0.01).double().mean(), (ro["sdf"].abs() < 0.02).double().mean(), sel.sum(), n * s]
    np.testing.assert_allclose(m.cpu().numpy(), [float(w) for w in want], rtol=1e-6)
    Rt = c2w[:3, :3].double().t()
    torch.testing.assert_close(imgs["normal_cam"].cpu().double(), (ro["normal"].double() @ Rt.t()), rtol=1e-5, atol=1e-6)
    dres = (gt - ro["depth"].reshape(-1)).abs()
    dres[gt < 1e-3] = 0
    assert torch.equal(imgs["depth_res"].cpu(), dres) and float(imgs["depth_res"][3]) > 0    # 1e-3: kept in the image
    empty_imgs, me = image_metrics(rod, torch.zeros(n, device=dev), gc.to(dev), c2w)
    me = me.cpu().numpy()
    assert np.isnan(me[:4]).all() and me[6] == 0
