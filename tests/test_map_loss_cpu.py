"""The float64 referee of the mapper's loss (tests/map_loss_restatement.py) is anchored on the reference's recorded batch,
its cases are shown to reach every branch with a margin, wrong variants of it are shown to miss the GPU test's bounds by
two orders of magnitude, and the unfused torch path of mapping_loss_sharded is compared with it in fp32 on the CPU --
including the shard without a single depth measurement, whose sdf gradient was 0 / 0."""
import os

import numpy as np
import pytest
import torch

import map_loss_restatement as R

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "mapper_loss.npz")


def test_restatement_reproduces_the_reference_mapper_fixture():
    """tests/golden/mapper_loss.npz = the reference's `Mapper.optimize_map` loss and the gradients its backward() left on
    the renderer's outputs, recorded in fp32: rtol 2e-5 on the loss, rtol 1e-4 / atol 1e-8 on the gradients (the bounds
    tests/test_neus_gpu.py already holds the kernel to on this fixture)."""
    g = {k: torch.from_numpy(np.asarray(v)) for k, v in np.load(GOLDEN).items()}
    wc, ws, we = (float(x) for x in g["weights"])
    n = g["sdf"].shape[0]
    c = dict(g, trunc=0.16, sparse=5, w_color=wc, w_sdf=ws, w_eikonal=we, uncertainty=True,
             count=float((g["rays_depth"] > 0).sum()), n_rays_global=float(n))
    ref = R.referee(c)
    loss, _ = R.total(c, ref)
    np.testing.assert_allclose(loss, float(g["loss"]), rtol=2e-5)
    for k in ("d_color", "d_depth", "d_sdf"):
        torch.testing.assert_close(ref[k].float(), g[k].reshape(ref[k].shape), rtol=1e-4, atol=1e-8, msg=lambda m: f"{k}: {m}")
    np.testing.assert_allclose(R.d_gradient_error(c), float(g["d_gradient_error"]), rtol=1e-6)


ALL = dict(R.CASES, too_wide=R.TOO_WIDE)


@pytest.mark.parametrize("name", list(ALL))
def test_no_case_sits_on_a_coin_flip(name):
    """In fp64: apart from the `boundary` case's placed samples nothing lies within 1e-5 of z == gt - trunc or of
    |gt - z| == trunc, and no front sample has |a - diff| <= 1e-4 max(1, |a|), so fp32 and fp64 take the same branches.
    (An exact tie a == diff is left out: where the loss passes, m >= 0, it needs pred <= 0 and pred >= gt - z > trunc > 0.
    For the same reason `diff > a > 0` does not exist in a front sample; its reachable form is diff > 0 > a.)"""
    c = ALL[name]
    mk = R.masks(c)
    t = R._f32(c["trunc"])
    free = ~c["placed"] & mk["valid"][:, None]
    assert float(((mk["bound"] - t).abs()[free]).min() if bool(free.any()) else 1.0) > 1e-5
    assert float(((mk["bound"].abs() - t).abs()[free]).min() if bool(free.any()) else 1.0) > 1e-5
    f = mk["front"]
    assert bool(((mk["a"] - mk["diff"]).abs() > 1e-4 * mk["a"].abs().clamp(min=1.0))[f].all())
    if name == "boundary":
        assert c["trunc"] == 0.125 and int(c["placed"].sum()) == 4 * 6
        on = c["placed"] & mk["valid"][:, None]
        assert bool((mk["bound"].abs()[on] == 0.125).all()) and bool(mk["near"][on].all()) and not bool(mk["front"][on].any())
    else:
        assert not bool(c["placed"].any())


def _count(c):
    mk = R.masks(c)
    f, nr, a, diff, m, arg, pred = (mk[k] for k in ("front", "near", "a", "diff", "m", "arg", "pred"))
    v = mk["valid"]
    dc = (c["color"] - c["rays_color"])[v]
    dd = (c["depth"].reshape(-1) - c["rays_depth"])[v]
    dv = c["depth_variance"].reshape(-1)[v]
    return dict(invalid=int((~v).sum()), clamped=int((f & (arg > 10)).sum()), at_clamp=int((f & (arg == 10)).sum()),
                pred_zero=int((f & (pred == 0)).sum()), m_negative=int((f & (m < 0)).sum()),
                m_zero=int((f & (m == 0)).sum()), diff_wins=int((f & (diff > 0) & (a < 0)).sum()),
                exp_wins=int((f & (a > 0) & (diff < 0) & (arg < 10)).sum()), diff_zero=int((nr & (diff == 0)).sum()),
                diff_pos=int((nr & (diff > 0)).sum()), diff_neg=int((nr & (diff < 0)).sum()),
                colour_equal=int((dc == 0).sum()), depth_equal=int((dd == 0).sum()),
                var_zero_residual=int(((dv == 0) & (dd != 0)).sum()), front=int(f.sum()), near=int(nr.sum()))


def test_every_named_branch_occurs():
    k = _count(R.CASES["branches"])
    floor = dict(invalid=3, clamped=8, at_clamp=8, pred_zero=50, m_negative=50, m_zero=50, diff_wins=50, exp_wins=50,
                 diff_zero=50, diff_pos=50, diff_neg=50, colour_equal=6, depth_equal=3, var_zero_residual=3)
    assert all(k[b] >= v for b, v in floor.items()), (k, floor)
    assert R.CASES["branches"]["sdf"].shape[1] == 72
    k = _count(R.CASES["boundary"])
    assert k["near"] == 5 * 9 and k["front"] == 5 * 3, k        # per valid ray: +-128 twice, +-127, +-1, 0 | 300, 129, 200
    k = _count(R.CASES["no_samples"])
    assert k["front"] == 0 and k["near"] == 0 and k["invalid"] == 1
    c = R.CASES["no_samples"]
    assert bool((c["z_vals"] > c["rays_depth"][:, None] + 0.16)[c["rays_depth"] > 0].all())
    assert sorted(tuple(R.CASES[f"widths-s{s}-n{n}"]["sdf"].shape[::-1]) for s, n in R.WIDTHS) == sorted(R.WIDTHS)
    for s, n in R.WIDTHS:
        k = _count(R.CASES[f"widths-s{s}-n{n}"])
        assert k["invalid"] == 0 and k["front"] + k["near"] >= (1 if s > 1 else 0), (s, n, k)
    assert sum(_count(R.CASES[f"widths-s{s}-n{n}"])["at_clamp"] for s, n in R.WIDTHS) >= 8
    c = R.CASES["sharded"]
    assert c["count"] == 3 * float((c["rays_depth"] > 0).sum()) and c["n_rays_global"] == 3 * 13
    c = R.CASES["empty_shard"]
    assert not bool((c["rays_depth"] > 0).any()) and c["count"] == 7
    c = R.CASES["no_uncertainty"]
    assert not c["uncertainty"] and _count(c)["var_zero_residual"] >= 1
    assert R.TOO_WIDE["sdf"].shape[1] == 129
    assert all(v["sdf"].shape[0] <= 64 and v["sdf"].shape[1] <= 128 for v in R.CASES.values())


def test_wrong_variants_miss_the_bounds():
    """Each subtly wrong loss, measured like a kernel output against the referee with the GPU test's bounds, exceeds a
    bound by a factor of at least 100 on some case (inf: a referee's exact zero is not zero, or a NaN)."""
    refs = {name: (R.referee(c), c) for name, c in R.CASES.items()}
    report = {}
    for v in R.VARIANTS:
        best = (0.0, None, None)
        for name, (ref, c) in refs.items():
            bad = R.referee(c, variant=v)
            bnd = R.bounds(c, ref, "kernel")
            for k in bnd:
                r = R.worst_ratio(bad[k], ref[k], bnd[k])
                if r > best[0]:
                    best = (r, name, k)
        report[v] = best
    lines = "\n".join(f"  {v}: x{r:.3g} over the bound of {k} in `{name}`" for v, (r, name, k) in report.items())
    print(lines)
    assert all(r >= 100 for r, _, _ in report.values()), "\n" + lines
    assert report["near_strict"][1] == "boundary" and report["local_count"][1] in ("sharded", "empty_shard"), "\n" + lines


# ------------------------------------------------------------------------------------- the unfused path, fp32, CPU ----
@pytest.fixture(scope="module")
def cpu_model():
    from go_slam_amd.neus import InstantNeuS
    return InstantNeuS({}, [[-1.0, 1.0]] * 3, device="cpu")


def test_shard_without_depth_has_finite_loss_and_zero_gradients(monkeypatch, cpu_model):
    """Every ray of the shard lacks a depth measurement while the other ranks hold 7 valid rays: the loss is the eikonal
    share alone, and the gradients w.r.t. colour, depth and sdf are exact zeros (the division by the LOCAL valid count
    0 used to put 0 / 0 into sdf.grad, and the gradient all-reduce then spread it)."""
    c = R.CASES["empty_shard"]
    loss, glob, ret = R.run_sharded(c, "cpu", False, monkeypatch, cpu_model)
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(glob))
    for k in ("color", "depth", "sdf"):
        assert bool((ret[k].grad == 0).all()), f"{k}.grad: {ret[k].grad.flatten()[:8]}"
    assert bool(torch.isfinite(ret["gradient_error"].grad).all())
    R.check_sharded(c, loss, glob, ret, "torch")


@pytest.mark.parametrize("name", [k for k in ALL if k != "empty_shard"])
def test_unfused_path_matches_the_referee_on_cpu(name, monkeypatch, cpu_model):
    c = ALL[name]
    R.check_sharded(c, *R.run_sharded(c, "cpu", False, monkeypatch, cpu_model), "torch")
