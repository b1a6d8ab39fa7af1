"""Mesh evaluation on the MI355X: NNIndex against the brute-force restatement bit for bit (d2 and index), against
cKDTree at 1.2 M points, registration_icp / eval_mesh against the restatement, and Mesher.__call__ end to end."""
import builtins
import sys
import types
import warnings

import numpy as np
import pytest
import torch

import mesh_eval_restatement as ER
from test_mesh_eval_cpu import rigid, room, sphere_mesh

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def check_nn(q, r, max_distance=None, transform=None):
    from go_slam_amd.neus.mesh_eval import NNIndex
    index = NNIndex(r, DEV)
    d2, idx = index.query(q, max_distance=max_distance, transform=transform)
    rd2, ridx = ER.nn(q, r, max_distance, transform)
    got_d2, got_idx = d2.cpu().numpy(), idx.cpu().numpy()
    assert np.array_equal(got_idx, ridx), np.flatnonzero(got_idx != ridx)[:10]
    assert np.array_equal(got_d2.view(np.int64), rd2.view(np.int64))      # bit for bit
    return index, got_d2, got_idx


def test_uniform_points(built_lib):
    g = np.random.default_rng(1)
    check_nn(g.uniform(-1.1, 1.1, (20000, 3)), g.uniform(-1, 1, (30000, 3)))


def test_surface_samples(built_lib):
    v, f = room(28)
    np.random.seed(5)
    r = ER.sample_surface(v, f, 20000)
    q = ER.sample_surface(v, f, 15000) + np.random.normal(scale=0.01, size=(15000, 3))
    check_nn(q, r)


def test_duplicates_and_ties(built_lib):
    g = np.random.default_rng(2)
    base = np.round(g.uniform(-1, 1, (500, 3)) * 8) / 8          # a lattice: many equal distances
    r = np.concatenate([base, base[::-1], base[:100]])          # exact duplicates at several indices
    q = np.concatenate([np.round(g.uniform(-1, 1, (3000, 3)) * 16) / 16, base[:200]])
    _, _, idx = check_nn(q, r)
    assert (idx < 500).mean() > 0.5


@pytest.mark.parametrize("kind", ["planar", "collinear", "single"])
def test_degenerate_reference_sets(built_lib, kind):
    g = np.random.default_rng(3)
    r = g.uniform(-1, 1, (4000, 3))
    if kind == "planar":
        r[:, 2] = 0.25
    elif kind == "collinear":
        r[:, 1:] = 0.5
    else:
        r = r[:1]
    check_nn(g.uniform(-1.5, 1.5, (3000, 3)), r)


def test_query_counts_one_and_zero(built_lib):
    g = np.random.default_rng(4)
    r = g.uniform(-1, 1, (1000, 3))
    check_nn(g.uniform(-1, 1, (1, 3)), r)
    from go_slam_amd.neus.mesh_eval import NNIndex
    d2, idx = NNIndex(r, DEV).query(np.zeros((0, 3)))
    assert d2.shape == (0,) and idx.shape == (0,)


def test_far_queries_take_the_fallback(built_lib):
    g = np.random.default_rng(6)
    r = g.uniform(0, 1, (50000, 3))
    index, _, _ = check_nn(g.uniform(0, 1, (2000, 3)), r)
    assert int(index.fallback.item()) == 0
    # 1000 cells out along the diagonal: each ring adds little and the bound grows slowly, so the cell budget runs out
    # (1000 cells out along one axis instead is settled by the first ring that meets the grid: the whole facing slab)
    far = g.uniform(0, 1, (700, 3)) + 1000.0 * index.h
    mixed = np.concatenate([far, g.uniform(0, 1, (300, 3)), -far])
    index, _, _ = check_nn(mixed, r)
    assert int(index.fallback.item()) >= 1400


def test_radius_boundary(built_lib):
    g = np.random.default_rng(7)
    r = np.round(g.uniform(-1, 1, (5000, 3)) * 64) / 64
    q = np.round(g.uniform(-1, 1, (5000, 3)) * 64) / 64 + np.array([0.0, 0.0, 0.0625])
    _, d2_all, _ = check_nn(q, r)
    rad = 0.0625                                 # dyadic: many queries sit exactly at d2 == r^2
    _, d2, idx = check_nn(q, r, max_distance=rad)
    at = d2_all == rad * rad
    assert at.sum() > 10 and np.all(idx[at] == -1) and np.all(np.isinf(d2[at]))
    assert np.all(idx[d2_all < rad * rad] >= 0)
    check_nn(q, r, max_distance=0.0)
    check_nn(q, r, max_distance=0.2)


def test_query_with_transform(built_lib):
    g = np.random.default_rng(8)
    r = g.uniform(-1, 1, (20000, 3))
    T = rigid(17.0, (1, -2, 0.5), (0.1, -0.3, 0.2))
    T[:3, :3] *= 1.1
    check_nn(g.uniform(-1, 1, (8000, 3)), r, transform=T)
    check_nn(g.uniform(-1, 1, (8000, 3)), r, transform=T, max_distance=0.05)


def _room_cloud(res):
    from go_slam_amd.neus.mesh import marching_cubes
    x = torch.linspace(-3.0, 3.0, res, device=DEV)
    X, Y, Z = torch.meshgrid(x, x, x, indexing="ij")
    walls = 2.8 - torch.maximum(torch.maximum(X.abs(), Y.abs()), (Z * 1.3).abs())
    table = torch.maximum(torch.maximum((X - 0.5).abs() - 0.6, (Y + 0.3).abs() - 0.4), (Z + 0.8).abs() - 0.05)
    u = -torch.minimum(walls, table)
    del X, Y, Z, walls, table
    v, f = marching_cubes(u, 0.0)
    return (v.double() / (res - 1) * 6.0 - 3.0), f


def test_1m_against_ckdtree(built_lib):
    from scipy.spatial import cKDTree
    from go_slam_amd.neus.mesh_eval import NNIndex
    v, _ = _room_cloud(512)
    n = min(v.shape[0], 1_200_000)
    r = v[:n].cpu().numpy()
    assert n > 1_000_000
    g = np.random.default_rng(9)
    q = r[g.permutation(n)] + g.normal(scale=0.01, size=(n, 3))
    d2, idx = NNIndex(r, DEV).query(q)
    d2, idx = d2.cpu().numpy(), idx.cpu().numpy()
    dist, j = cKDTree(r).query(q, workers=16)
    np.testing.assert_allclose(np.sqrt(d2), dist, rtol=1e-12, atol=0)
    assert np.mean(idx == j) > 0.999
    far = idx != j
    if far.any():   # a different index must be an equally near point
        np.testing.assert_allclose(((q[far] - r[j[far]]) ** 2).sum(1), d2[far], rtol=1e-12)


def test_two_runs_are_bitwise_identical(built_lib):
    from go_slam_amd.neus.mesh_eval import NNIndex
    g = np.random.default_rng(10)
    r = g.uniform(-1, 1, (200000, 3))
    q = np.concatenate([g.uniform(-1.2, 1.2, (200000, 3)), g.uniform(50, 60, (2000, 3))])
    a = NNIndex(r, DEV).query(q)
    b = NNIndex(r, DEV).query(q)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("scale", [1.0, 1.2])
def test_icp_matches_restatement(built_lib, scale):
    from go_slam_amd.neus.mesh_eval import registration_icp
    v, _ = room(40)
    T_true = rigid(4.0, (0.2, 1.0, -0.3), (0.04, -0.03, 0.02))
    S = np.diag([scale, scale, scale, 1.0])
    src = ER.transform_points(v, np.linalg.inv(T_true @ S))[::2]
    init = S @ rigid(0.5, (1, 0, 0), (0.01, 0, 0))
    res = registration_icp(src, v, 0.1, init)
    T, fit, rmse, it = ER.icp(src, v, 0.1, init)
    np.testing.assert_allclose(res.transformation, T, rtol=0, atol=1e-9)
    assert res.iterations == it and res.fitness == fit
    np.testing.assert_allclose(res.inlier_rmse, rmse, rtol=1e-9, atol=1e-15)


def test_icp_without_correspondences(built_lib):
    from go_slam_amd.neus.mesh_eval import registration_icp
    res = registration_icp(np.zeros((5, 3)), np.full((4, 3), 10.0), 0.1)
    assert np.array_equal(res.transformation, np.eye(4)) and res.fitness == 0.0 and res.inlier_rmse == 0.0


def test_eval_mesh_matches_restatement(built_lib, tmp_path):
    from go_slam_amd.neus.mesh import Mesh
    from go_slam_amd.neus.mesh_eval import eval_mesh
    v, f = room(40)
    gv, gf = sphere_mesh(1.0, 48)
    gv = gv * 1.2
    np.random.seed(43)
    got = eval_mesh(Mesh(v, f), Mesh(gv, gf), N3d=20000, dist_th=0.05, out_path=str(tmp_path / "m.txt"))
    np.random.seed(43)
    ref = ER.eval_mesh(v, f, gv, gf, 20000, 0.05)
    assert got.keys() == ref.keys()
    for k in ref:
        assert got[k] == ref[k], k
    assert (tmp_path / "m.txt").read_text().count("\n") == 9


def _cfg(eval_rec, gt_path):
    return {"meshing": {"resolution": 96, "level_set": 0.0, "remove_small_geometry_threshold": 0.2,
                        "get_largest_components": False, "eval_rec": eval_rec, "n_points_to_eval": 2000,
                        "mesh_threshold_to_eval": 0.05, "gt_mesh_path": gt_path, "forecast_radius": 25},
            "mapping": {"device": DEV}}


@pytest.mark.parametrize("eval_rec", [True, False])
def test_mesher_call_aligns_and_evaluates(built_lib, tmp_path, monkeypatch, eval_rec):
    from test_mesh_gpu import _model
    from go_slam_amd.depth_video import DepthVideo
    from go_slam_amd.neus.mesher import Mesher
    real_import = builtins.__import__

    def guarded(name, *a, **k):
        if name.split(".")[0] in ("open3d", "pyrender", "trimesh"):
            raise ImportError(name)
        return real_import(name, *a, **k)
    monkeypatch.setattr(builtins, "__import__", guarded)
    for name in ("open3d", "pyrender", "trimesh"):
        monkeypatch.setitem(sys.modules, name, None)
    model, _ = _model()
    gt = model.extract_geometry(64, 0.0, save_path=None)
    gt_path = str(tmp_path / "gt.ply")
    gt.export(gt_path)
    video = DepthVideo(6, 8, buffer=8, device=DEV, full_res=True)
    n = 5
    yy, xx = torch.meshgrid(torch.arange(48.0), torch.arange(64.0), indexing="ij")
    bump = 0.5 + 0.1 * torch.sin(xx / 9.0) * torch.cos(yy / 7.0)
    for i in range(n):
        video.poses[i] = torch.tensor([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0])
        video.disps_up[i] = bump
        video.timestamp[i] = float(i)
    video.intrinsics[:n] = torch.tensor([5.0, 5.0, 4.0, 3.0])
    video.counter.value = n
    slam = types.SimpleNamespace(output=str(tmp_path), mapping_net=model, video=video,
                                 reload_map=torch.zeros(1).int(), verbose=False, H=48, W=64, fx=40.0, fy=40.0,
                                 cx=32.0, cy=24.0)
    m = Mesher(_cfg(eval_rec, gt_path), None, slam)
    trans_init = rigid(1.0, (0, 0, 1), (0.01, 0.0, 0.0))
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        m(the_end=True, trans_init=trans_init)
    assert not [w for w in caught if "mesh" in str(w.message).lower()], [str(w.message) for w in caught]
    assert (tmp_path / "mesh" / "final_raw_mesh.ply").exists()
    assert (tmp_path / "mesh" / "aligned_mesh.ply").exists()
    assert (tmp_path / "mesh" / "forecast_aligned_mesh.ply").exists()
    assert (tmp_path / "metrics_mesh.txt").exists() == eval_rec
    if eval_rec:
        assert "F-score" in (tmp_path / "metrics_mesh.txt").read_text()
