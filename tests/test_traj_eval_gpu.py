"""gs_traj_world / gs_ape_moments / gs_ape_stats on the GPU against tests/traj_eval_restatement.py.

Tolerance: the restatement carries a forward-error bound for every number it returns (operation count along the longest
chain x 2^-53 x the sum of the absolute terms, with the errors of earlier passes carried along; see its docstring).
Kernel and restatement both stay within that bound of the exact value, so they may differ by twice the bound; a number
whose bound is zero (the count, -1 markers, exact cases) must be equal.  No constant is chosen.

Sizes: 3 and 4 (fewer frames than a wave, even and odd), 63 / 64 / 65 (a wave's edges), 257 (two blocks, the second
with one frame), 1031 (five blocks, ragged last one)."""
import functools

import numpy as np
import pytest
import torch

import traj_eval_restatement as TR
from go_slam_amd import eval_ate

pytestmark = pytest.mark.gpu

SIZES = [3, 4, 63, 64, 65, 257, 1031]
ALIGN_CASES = ["walk", "planar", "reflection", "offset_1e3", "scale_0.1", "scale_10", "nan_gt_rows"]
STATS_CASES = ["all_equal", "repeated"]


def _rotation(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


@functools.lru_cache(maxsize=None)
def make_case(name, n):
    """(est [n,3], ref [n,3], mask or None), fp64, read-only"""
    rng = np.random.default_rng(1000 * SIZES.index(n) + (ALIGN_CASES + STATS_CASES).index(name))
    ref = np.cumsum(rng.normal(size=(n, 3)) * 0.05, axis=0)
    noise = rng.normal(size=(n, 3)) * 0.01
    mask = None
    if name == "walk":
        est = (0.9 * (_rotation(rng) @ ref.T)).T + np.array([0.3, -1.0, 2.0]) + noise
    elif name == "planar":              # z exactly constant in both sets: a rank-2 covariance
        ref[:, 2] = 0.0
        est = ref * 1.1 + noise
        est[:, 2] = 0.0
    elif name == "reflection":
        ref = rng.normal(size=(n, 3))
        est = ref * np.array([1.0, 1.0, -1.0]) + noise
    elif name == "offset_1e3":          # a kilometre from the origin, millimetre noise: what the centred pass is for
        ref = ref + 1.0e3
        est = ref + rng.normal(size=(n, 3)) * 1e-3
    elif name in ("scale_0.1", "scale_10"):
        est = (float(name.split("_")[1]) * (_rotation(rng) @ ref.T)).T + noise
    elif name == "nan_gt_rows":         # GT rows that must never be read: the first, a middle one, the last
        est = ref + noise
        mask = np.ones(n, dtype=bool)
        mask[[0, n // 2, n - 1]] = False
        ref = ref.copy()
        ref[~mask] = np.nan
    elif name == "all_equal":           # |ref - est| = 0.5 exactly in every frame
        ref = np.round(ref * 64.0)
        est = ref - np.array([0.5, 0.0, 0.0])
    elif name == "repeated":            # four distinct errors, each many times over
        ref = np.round(ref * 64.0)
        est = ref - np.outer(np.array([0.25, 0.5, 0.5, 0.75, 0.25, 1.0])[np.arange(n) % 6], [0.0, 1.0, 0.0])
    for a in (est, ref):
        a.setflags(write=False)
    return est, ref, mask


def _gpu(a, dtype=torch.float64):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0", dtype)


def _close(got, want, bound, what):
    got, want, bound = np.asarray(got, dtype=np.float64), np.asarray(want), np.asarray(bound)
    both_nan = np.isnan(got) & np.isnan(want)
    diff = np.where(both_nan, 0.0, np.abs(got - want))
    worst = int(np.argmax(diff - 2 * np.where(both_nan, 0.0, bound)))
    print(f"{what}: max |diff| {diff.max():.3e}, bound there {np.ravel(bound)[worst]:.3e}")
    assert (diff <= 2 * np.where(both_nan, 0.0, bound)).all(), (what, np.ravel(got)[worst], np.ravel(want)[worst],
                                                                 np.ravel(bound)[worst])


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", ALIGN_CASES)
def test_alignment_and_statistics(built_lib, name, n):
    from go_slam_amd import traj_eval
    est, ref, mask = make_case(name, n)
    m_ref, m_bound = TR.ape_moments(est, ref, mask)
    m = traj_eval.ape_moments(_gpu(est), _gpu(ref), _gpu(mask, torch.bool))
    assert torch.equal(m, traj_eval.ape_moments(_gpu(est), _gpu(ref), _gpu(mask, torch.bool)))      # run to run
    m = m.cpu().numpy()
    assert m[0] == m_ref[0] == (n if mask is None else mask.sum())
    _close(m, m_ref, m_bound, "moments")
    if m[0] < 3:      # fewer than three valid frames: no similarity; the same error as eval_ate's
        with pytest.raises(ValueError, match="degenerate covariance rank"):
            traj_eval.ape(_gpu(est), _gpu(ref), _gpu(mask, torch.bool))
        if m[0] >= 1:
            with pytest.raises(ValueError, match="degenerate covariance rank"):
                eval_ate.umeyama_alignment(est[mask].T, ref[mask].T)
        return
    # the statistics for ONE similarity, handed to both sides: the host step in between is NumPy on both
    R, t, c = traj_eval.umeyama_from_moments(m)
    e_ref, s_ref, e_bound, s_bound = TR.ape_stats(est, ref, c * R, t, mask)
    err, stats = traj_eval.ape_stats(_gpu(est), _gpu(ref), c * R, t, _gpu(mask, torch.bool))
    err2, stats2 = traj_eval.ape_stats(_gpu(est), _gpu(ref), c * R, t, _gpu(mask, torch.bool))
    assert torch.equal(err, err2) and torch.equal(stats, stats2)
    _close(err.cpu().numpy(), e_ref, e_bound, "errors")
    _close(stats.cpu().numpy(), s_ref, s_bound, "statistics")
    # end to end, alignment included, against the restatement and against eval_ate on the valid rows
    full = traj_eval.ape(_gpu(est), _gpu(ref), _gpu(mask, torch.bool))
    want = TR.ape(est, ref, mask)
    sel = slice(None) if mask is None else mask
    rmse, info = eval_ate.ate_rmse(est[sel], ref[sel])
    for k in traj_eval.STAT_NAMES:
        _close(full[k], want[k], want["bound"][k], "end to end " + k)
    for k, v in (("rmse", rmse), ("mean", info["mean"]), ("median", info["median"]), ("max", info["max"])):
        _close(full[k], v, want["bound"][k], "eval_ate " + k)
    assert full["count"] == want["count"]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", STATS_CASES)
def test_median_ties(built_lib, name, n):
    """equal and repeated errors: ranks are broken by index, so exactly one frame owns each middle rank"""
    from go_slam_amd import traj_eval
    est, ref, _ = make_case(name, n)
    e_ref, s_ref, e_bound, s_bound = TR.ape_stats(est, ref, np.eye(3), np.zeros(3))
    err, stats = traj_eval.ape_stats(_gpu(est), _gpu(ref), np.eye(3), np.zeros(3))
    err, stats = err.cpu().numpy(), stats.cpu().numpy()
    assert (err == e_ref).all()                                      # exact inputs: 0.25, 0.5, 0.75, 1 come out exactly
    assert stats[2] == s_ref[2] == np.median(e_ref) and stats[3] == e_ref.min() and stats[4] == e_ref.max()
    _close(stats, s_ref, s_bound, "statistics")
    if name == "all_equal":
        assert stats[0] == stats[1] == stats[2] == 0.5 and stats[6] == 0.0


@pytest.mark.parametrize("n", SIZES)
def test_traj_world(built_lib, n):
    from go_slam_amd import traj_eval
    g = torch.Generator().manual_seed(n)
    q = torch.nn.functional.normalize(torch.randn(n, 4, generator=g), dim=1)
    w2c = torch.cat([torch.randn(n, 3, generator=g) * 3.0, q], dim=1)
    comp = torch.cat([torch.randn(3, generator=g), torch.nn.functional.normalize(torch.randn(4, generator=g), dim=0)])
    tq_ref, mat_ref, b_tq, b_mat = TR.traj_world(w2c.numpy(), comp.numpy())
    tq, mat = traj_eval.world_poses(w2c.cuda(), comp.cuda())
    tq2, mat2 = traj_eval.world_poses(w2c.cuda(), comp.cuda())
    assert torch.equal(tq, tq2) and torch.equal(mat, mat2)
    assert tq.dtype == mat.dtype == torch.float64 and mat.shape == (n, 4, 4)
    _close(tq.cpu().numpy(), tq_ref, b_tq, "tq")
    _close(mat.cpu().numpy(), mat_ref, b_mat, "matrix")
    assert (mat[:, 3].cpu() == torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=torch.float64)).all()
    assert torch.equal(mat[:, :3, 3], tq[:, :3])


def test_degenerate_input_raises_like_eval_ate(built_lib):
    from go_slam_amd import traj_eval
    line = np.outer(np.arange(65.0), [1.0, 0.0, 0.0]) + np.array([0.5, 2.0, -3.0])      # collinear, exactly rank 1
    two = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]])
    for pts in (line, two):
        with pytest.raises(ValueError) as mine:
            traj_eval.ape(_gpu(pts), _gpu(pts))
        with pytest.raises(ValueError) as theirs:
            eval_ate.umeyama_alignment(pts.T, pts.T)
        assert str(mine.value) == str(theirs.value)
    with pytest.raises(ValueError, match="degenerate covariance rank"):
        traj_eval.ape(_gpu(line), _gpu(line), torch.zeros(65, dtype=torch.bool, device="cuda:0"))
