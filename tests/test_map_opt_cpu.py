"""The fp64 restatement of the mapper step's kernels (tests/map_opt_restatement.py) against the code it restates --
clip_grad_norm_ + torch.optim.AdamW, the unfused backward's Gram slicing, MapTrainer's torch form of the batch counts,
gs_map_gram_blocks -- all without a GPU."""
import types

import numpy as np
import pytest
import torch

import map_opt_restatement as R

HYPER = dict(betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)


def _torch_clip_adamw(params, grads, lrs, max_norm=35.0):
    """the reference's step (src/mapping.py:55-58,135-137) on float64 CPU tensors"""
    ps = [torch.nn.Parameter(torch.tensor(p, dtype=torch.float64)) for p in params]
    opt = torch.optim.AdamW([{"params": [p], "lr": lr} for p, lr in zip(ps, lrs)], **HYPER)
    for gs in grads:
        for p, g in zip(ps, gs):
            p.grad = torch.tensor(g, dtype=torch.float64)
        torch.nn.utils.clip_grad_norm_(ps, max_norm, error_if_nonfinite=False)
        opt.step()
    st = [opt.state[p] for p in ps]
    return ([p.detach().numpy() for p in ps], [s["exp_avg"].numpy() for s in st],
            [s["exp_avg_sq"].numpy() for s in st])


def _problem(seed, scale, n=(300, 57), steps=4):
    rng = np.random.default_rng(seed)
    params = [rng.standard_normal(k) for k in n]
    grads = [[rng.standard_normal(k) * scale for k in n] for _ in range(steps)]
    return params, grads


@pytest.mark.parametrize("scale,active", [(5.0, True), (0.05, False)])
def test_clip_adamw_equals_clip_grad_norm_and_torch_adamw(scale, active):
    params, grads = _problem(1, scale)
    norms = [np.sqrt(sum((g * g).sum() for g in gs)) for gs in grads]
    assert all((nm > 35.0) == active for nm in norms), norms
    lrs = [1e-2, 1e-3]
    p, m, v, bounds = R.clip_adamw(params, grads, lrs, **HYPER)
    tp, tm, tv = _torch_clip_adamw(params, grads, lrs)
    for i in range(2):
        np.testing.assert_allclose(p[i], tp[i], rtol=1e-13, atol=1e-15)
        np.testing.assert_allclose(m[i], tm[i], rtol=1e-13, atol=1e-18)
        np.testing.assert_allclose(v[i], tv[i], rtol=1e-13, atol=1e-20)
        bp, bm, bv = bounds[i]
        assert (bp > 0).all() and (bm > 0).all() and (bv > 0).all()


def test_clip_adamw_inf_gradient_zeroes_the_finite_ones():
    params, grads = _problem(2, 1.0, steps=1)
    grads[0][1][7] = np.inf
    lrs = [1e-2, 1e-3]
    p, m, v, _ = R.clip_adamw(params, grads, lrs, **HYPER)
    tp, tm, tv = _torch_clip_adamw(params, grads, lrs)
    for i in range(2):
        assert R.same_nonfinite(p[i], tp[i]) and R.same_nonfinite(m[i], tm[i]) and R.same_nonfinite(v[i], tv[i])
        ok = np.isfinite(tp[i])
        np.testing.assert_allclose(p[i][ok], tp[i][ok], rtol=1e-13, atol=0)
    bad = np.zeros(57, bool)
    bad[7] = True
    assert np.isnan(p[1][bad]).all() and np.isfinite(p[1][~bad]).all() and np.isfinite(p[0]).all()
    # the clip coefficient is 0: every finite gradient became 0, so m = (1 - b1) * 0 and p only decays and steps by 0
    assert (m[0] == 0).all() and (m[1][~bad] == 0).all()
    np.testing.assert_allclose(p[0], params[0] * (1 - 1e-2 * 0.01), rtol=1e-15)


def test_clip_adamw_nan_gradient_makes_every_parameter_nan():
    params, grads = _problem(3, 1.0, steps=2)
    grads[1][0][11] = np.nan
    lrs = [1e-2, 1e-3]
    p, m, v, _ = R.clip_adamw(params, grads, lrs, **HYPER)
    tp, tm, tv = _torch_clip_adamw(params, grads, lrs)
    for i in range(2):
        assert np.isnan(tp[i]).all() and np.isnan(p[i]).all() and np.isnan(m[i]).all() and np.isnan(v[i]).all()
    assert np.isnan(R.clip_coef(float("nan"), 35.0)) and R.clip_coef(float("inf"), 35.0) == 0.0
    assert R.clip_coef(1.0, 35.0) == 1.0


def test_post_index_map_equals_the_unfused_backward_slicing():
    from go_slam_amd.neus.instant_neus import _gram_dense_grads
    g = torch.Generator().manual_seed(4)
    G = torch.randn(40, 160, generator=g, dtype=torch.float64) * 10.0 ** torch.randint(-3, 4, (40, 160), generator=g)
    w, b, cB = _gram_dense_grads(G)
    want = torch.cat([w.reshape(-1), b.reshape(-1), cB.reshape(-1)]).numpy()
    assert want.shape == (R.N_W + R.N_B + R.N_CB,)
    assert np.array_equal(R.post_dense(G.numpy()), want)


def test_post_reads_only_entries_the_gram_kernel_writes():
    written = R.gram_written().numpy()
    assert all(written[r, c] for e in R.POST_ENTRIES for r, c in e)
    assert not written[32:40, 32:64].any() and written.sum() == 32 * 64 + 8 * 128
    rng = np.random.default_rng(5)
    chunks = np.where(written, rng.standard_normal((3, 40, 160)), np.nan)
    out, bnd = R.post(chunks, 1 / 128, rng.standard_normal((2, R.N_MLP)), 0.5, 0.3, 20.0, 10.0,
                      rng.standard_normal(5), rng.random(5), 0.1, 72, np.array([5.0, 5.0, 3.0]))
    assert np.isfinite(out).all() and np.isfinite(bnd).all() and (bnd[:R.OFF_LOSS] >= 0).all()
    np.testing.assert_allclose(out[R.OFF_W:R.OFF_VAR], R.post_dense(np.nansum(chunks, 0)) / 128, rtol=1e-15)
    assert out[R.OFF_VAR] == 0.5 * 10.0 * 20.0                          # exp(3) is inside the clamp
    assert R.post(chunks, 1 / 128, np.zeros((1, R.N_MLP)), 0.5, -2.0, 20.0, 10.0, np.zeros(1), np.zeros(1), 0.1, 72,
                  np.ones(3))[0][R.OFF_VAR] == 0.0                         # exp(-20) < 1e-6: clamped, no gradient


def test_gram_split_covers_every_group_once(built_lib):
    from go_slam_amd import _lib
    L = _lib.lib()
    for k in range(1, 20001):
        n_rows = 16 * k
        split = R.gram_split(n_rows)
        assert len(split) == R.gram_blocks(n_rows) == L.gs_map_gram_blocks(n_rows), n_rows
        lo = np.array([a for a, _ in split])
        hi = np.array([b for _, b in split])
        assert lo[0] == 0 and hi[-1] == n_rows and (hi >= lo).all(), n_rows
        # contiguous and in order: every row in exactly one workgroup
        assert (lo[1:] == hi[:-1]).all(), n_rows
        per = 16 * -(-k // len(split))
        assert ((hi - lo) <= per).all() and (hi - lo)[:-1].max(initial=per) == per, n_rows
    for n_rows in (263232, 294912, 2359296, 4096 * 16, 4112 * 16):
        assert R.gram_blocks(n_rows) == L.gs_map_gram_blocks(n_rows)


def test_gram_split_sizes_with_empty_workgroups():
    split = R.gram_split(263232)                  # 3656 rays x 72 samples: 16452 groups, 257 -> 256 workgroups of 65
    assert len(split) == 256
    sizes = [(b - a) // 16 for a, b in split]
    assert sizes[:253] == [65] * 253 and sizes[253] == 16452 - 253 * 65 and sizes[254:] == [0, 0]
    # empty trailing workgroups start far below the 256-workgroup cap: 4225 groups -> 66 workgroups of 65, the last
    # one empty
    empties = [n for n in range(16, 16 * 20001, 16) if any(a == b for a, b in R.gram_split(n))]
    assert empties[0] == 67600 and R.gram_split(67600)[-1] == (67600, 67600) and 263232 in empties
    assert R.gram_split(2359296)[-1] == (2359296 - 576 * 16, 2359296)


@pytest.mark.parametrize("depths", [
    [], [1.0], [0.0], [-1.0], [-3.0, -2.0], [0.0, 0.0, 0.0],
    [1.5, 0.0, -2.0, np.inf, 3.0], [-np.inf, -1.0], [np.nan], [2.0, np.nan, 5.0, -1.0, 0.0],
    [np.nan, np.inf, -np.inf, 0.0, 1.0],
])
def test_prep_counts_equal_maptrainer_torch_form(depths):
    from go_slam_amd.neus.mapper import MapTrainer
    d = torch.tensor(depths, dtype=torch.float32)
    got = MapTrainer._counts(types.SimpleNamespace(sharded=True), d).double().numpy()
    np.testing.assert_array_equal(R.counts(np.asarray(depths, np.float32)), got)


def test_prep_counts_large_random_with_specials():
    from go_slam_amd.neus.mapper import MapTrainer
    rng = np.random.default_rng(6)
    for n, special in ((8193, None), (32768, np.nan), (1023, np.inf), (1023, -np.inf)):
        d = rng.uniform(-2.0, 8.0, n).astype(np.float32)
        d[rng.integers(0, n, n // 10)] = 0.0
        if special is not None:
            d[rng.integers(0, n)] = special
        got = MapTrainer._counts(types.SimpleNamespace(sharded=True), torch.from_numpy(d)).double().numpy()
        np.testing.assert_array_equal(R.counts(d), got)


def test_prep_restatement_transpose_and_gather():
    from go_slam_amd.neus.tcnn_compat import _mlp_fragment_index32, _pack_mlp_fragments
    rng = np.random.default_rng(7)
    sdf_w = rng.standard_normal((32, 35)).astype(np.float32)
    W = torch.from_numpy(rng.standard_normal(10240).astype(np.float16))
    idx = _mlp_fragment_index32(torch.device("cpu"))
    out = R.prep(np.ones(4, np.float32), 0.3, 10.0, 0.1, 72, sdf_w=sdf_w, mlp16=W.numpy(), frag_index=idx.numpy())
    for lf in range(32):
        for o in range(32):
            assert out["sdf_wt"][lf * 32 + o] == sdf_w[o, 3 + lf]
    assert np.array_equal(out["mlp_wpack"].view(np.int16), _pack_mlp_fragments(W).reshape(-1).numpy().view(np.int16))
    assert out["counts"].tolist() == [4.0, 4.0, 1.0] and out["d_gerr"].shape == (4,)
    assert out["inv_s"] == pytest.approx(np.exp(3.0), rel=1e-6)
    assert R.inv_s(-2.0, 10.0) == 1e-6 and R.inv_s(1.5, 10.0) == 1e6


def test_sqnorm_restatement():
    rng = np.random.default_rng(8)
    g16 = (rng.standard_normal(1000) * 100).astype(np.float16)
    g32 = rng.standard_normal(77).astype(np.float32)
    want = float((torch.from_numpy(g16).double() / 128).pow(2).sum() + torch.from_numpy(g32).double().pow(2).sum())
    assert R.sqnorm(g16, 1 / 128, g32) == pytest.approx(want, rel=1e-14)
    g16[3] = np.inf
    assert R.sqnorm(g16, 1 / 128, g32) == np.inf
    g16[4] = np.nan
    assert np.isnan(R.sqnorm(g16, 1 / 128, g32))
    assert R.sqnorm_blocks(0, 1) == 1 and R.sqnorm_blocks(12599920, 11492) == 256
