"""tests/traj_eval_restatement.py (the CPU restatement of gs_traj_world / gs_ape_moments / gs_ape_stats) against
go_slam_amd.eval_ate, against lietorch_shim's fp32 composition and against cases whose answer is known in closed form.
No GPU: this is what makes the restatement a reference for tests/test_traj_eval_gpu.py."""
import numpy as np
import pytest
import torch

import traj_eval_restatement as TR
from go_slam_amd import eval_ate
from go_slam_amd.lietorch_shim import SE3


def _rotation(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _walk(rng, n, step=0.05):
    return np.cumsum(rng.normal(size=(n, 3)) * step, axis=0)


@pytest.mark.parametrize("n", [3, 16, 257, 1031])
def test_restatement_matches_eval_ate_on_noisy_trajectories(n):
    rng = np.random.default_rng(n)
    ref = _walk(rng, n)
    est = (0.7 * (_rotation(rng) @ ref.T)).T + np.array([0.3, -1.0, 2.0]) + rng.normal(size=(n, 3)) * 0.01
    got = TR.ape(est, ref)
    rmse, info = eval_ate.ate_rmse(est, ref)
    err = np.linalg.norm(ref - (info["scale"] * (info["rotation"] @ est.T).T + info["translation"]), axis=1)
    want = {"rmse": rmse, "mean": info["mean"], "median": info["median"], "max": info["max"], "min": err.min(),
            "sse": (err ** 2).sum(), "std": err.std()}
    for k, v in want.items():
        # both evaluations obey the restatement's end-to-end bound against the exact value
        assert abs(got[k] - v) <= 2 * got["bound"][k], (k, got[k], v, got["bound"][k])
        assert got["bound"][k] < 1e-9 * max(1.0, abs(v))                          # and the bound says something
    assert np.allclose(got["rotation"], info["rotation"], atol=1e-10) and abs(got["scale"] - info["scale"]) < 1e-10


def test_mask_equals_dropping_the_rows():
    rng = np.random.default_rng(3)
    ref = _walk(rng, 65)
    est = ref + rng.normal(size=ref.shape) * 0.02
    mask = np.ones(65, dtype=bool)
    mask[[0, 31, 64]] = False
    bad = ref.copy()
    bad[~mask] = np.nan                                              # never read
    got = TR.ape(est, bad, mask)
    rmse, info = eval_ate.ate_rmse(est[mask], ref[mask])
    assert got["count"] == 62 and abs(got["rmse"] - rmse) <= 2 * got["bound"]["rmse"]
    assert (got["errors"][~mask] == -1).all() and (got["errors"][mask] >= 0).all()


def test_known_sim3_is_recovered_with_zero_error():
    rng = np.random.default_rng(11)
    est = _walk(rng, 64, 0.2)
    R, c, t = _rotation(rng), 2.5, np.array([1.0, -2.0, 0.5])
    ref = (c * (R @ est.T)).T + t
    got = TR.ape(est, ref)
    assert np.allclose(got["rotation"], R, atol=1e-12) and abs(got["scale"] - c) < 1e-12
    assert np.allclose(got["translation"], t, atol=1e-12)
    assert got["max"] < 1e-12 and got["rmse"] <= got["max"] and got["min"] >= 0.0


def test_mirrored_points_take_the_reflection_branch():
    rng = np.random.default_rng(12)
    est = rng.normal(size=(65, 3))
    ref = est * np.array([1.0, 1.0, -1.0])                           # a mirror image: no rotation maps one to the other
    m, _ = TR.ape_moments(est, ref)
    Um, D, Vt = np.linalg.svd(m[7:16].reshape(3, 3))
    assert np.linalg.det(Um) * np.linalg.det(Vt) < 0
    R, t, c = TR.umeyama_from_moments(m)
    assert abs(np.linalg.det(R) - 1.0) < 1e-12                       # still a proper rotation
    R2, t2, c2 = eval_ate.umeyama_alignment(est.T, ref.T)
    assert np.allclose(R, R2, atol=1e-12) and abs(c - c2) < 1e-12 and TR.ape(est, ref)["rmse"] > 0.1


def test_degenerate_inputs_raise_like_eval_ate():
    # collinear along an axis: the centred y and z are exactly zero, so the covariance has exactly one non-zero singular
    # value (a slanted line leaves ~1e-15 there, which eval_ate's absolute threshold, like evo's, lets through)
    line = np.outer(np.arange(5.0), [1.0, 0.0, 0.0]) + np.array([0.5, 2.0, -3.0])
    for est, ref, mask in ((line, line, None), (np.zeros((4, 3)), np.zeros((4, 3)), np.zeros(4, dtype=bool))):
        with pytest.raises(ValueError, match="degenerate covariance rank"):
            TR.ape(est, ref, mask)
    with pytest.raises(ValueError, match="degenerate covariance rank"):
        eval_ate.umeyama_alignment(line.T, line.T)


def test_median_rule():
    ref = np.zeros((6, 3))
    est = np.zeros((6, 3))
    est[:, 0] = [3.0, 1.0, 1.0, 2.0, 5.0, 1.0]
    mask = np.ones(6, dtype=bool)
    for n, want in ((6, 1.5), (5, 2.0)):                             # even: the two middle ranks averaged; odd: the middle
        err, stats, _, _ = TR.ape_stats(est[:n], ref[:n], np.eye(3), np.zeros(3), mask[:n])
        assert stats[2] == want == np.median(err) and stats[3] == 1.0 and stats[4] == err.max()
    err, stats, _, _ = TR.ape_stats(np.ones((4, 3)), ref[:4], np.eye(3), np.zeros(3))
    assert stats[2] == stats[3] == stats[4] == np.sqrt(3.0) and stats[6] == 0.0      # all equal: ties by index


def test_reduction_order_is_the_documented_one():
    rng = np.random.default_rng(0)
    x = rng.normal(size=1031) * 10.0 ** rng.integers(-8, 8, size=1031)
    pad = np.zeros(5 * 256)
    pad[:1031] = x
    parts = []
    for b in range(5):
        red = pad[b * 256:(b + 1) * 256].copy()
        w = 128
        while w:
            for t in range(w):
                red[t] = red[t] + red[t + w]
            w //= 2
        parts.append(red[0])
    acc = np.zeros(256)
    acc[:5] = parts
    w = 128
    while w:
        for t in range(w):
            acc[t] = acc[t] + acc[t + w]
        w //= 2
    assert TR.reduce_fixed(x) == acc[0]
    assert abs(TR.reduce_fixed(x) - float(np.sum(x.astype(np.longdouble)))) <= TR.chain_length(1031) * TR.U * np.abs(x).sum()


def test_traj_world_matches_the_fp32_composition():
    g = torch.Generator().manual_seed(2)
    q = torch.nn.functional.normalize(torch.randn(65, 4, generator=g), dim=1)
    w2c = torch.cat([torch.randn(65, 3, generator=g) * 2.0, q], dim=1)
    comp = torch.cat([torch.randn(3, generator=g), torch.nn.functional.normalize(torch.randn(4, generator=g), dim=0)])
    tq, mat, b_tq, b_mat = TR.traj_world(w2c.numpy(), comp.numpy())
    ref = SE3(comp[None].double()) * SE3(w2c.double()).inv()
    assert np.abs(tq - ref.data.numpy()).max() <= 2 * b_tq.max() and b_tq.max() < 1e-13
    assert np.abs(mat - ref.matrix().numpy()).max() <= 2 * b_mat.max()
    f32 = SE3(comp[None]) * SE3(w2c).inv()
    assert np.abs(tq - f32.data.double().numpy()).max() < 64 * 2.0 ** -24 * 8.0     # the fp32 route agrees to fp32
    assert (mat[:, 3] == [0, 0, 0, 1]).all()
    assert np.abs(mat[:, :3, :3] @ mat[:, :3, :3].transpose(0, 2, 1) - np.eye(3)).max() < 1e-5
