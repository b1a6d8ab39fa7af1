"""Mesh culling on the MI355X against the CPU restatements (tests/cull_restatement.py): depth maps, visibility masks,
face components and areas, the hull pre-filter and OBB, and Mesher.cull_mesh / Mesher.__call__ end to end."""
import builtins
import sys
import types

import numpy as np
import pytest
import torch

import cull_restatement as CR
from test_mesher_cpu import sphere

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """c2w, OpenCV axes (x right, y down, z forward)."""
    eye, target, up = (np.asarray(a, np.float64) for a in (eye, target, up))
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross(z, up)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = x, y, z, eye
    return m


def blob_mesh(seed=0, n=28):
    """A marching-cubes mesh of a smooth random field (many components, open boundaries) in world units."""
    from go_slam_amd.neus.mesh import marching_cubes
    g = torch.Generator().manual_seed(seed)
    u = torch.nn.functional.interpolate(torch.randn(1, 1, 5, 6, 5, generator=g), size=(n, n, n), mode="trilinear",
                                        align_corners=True)[0, 0]
    v, f = marching_cubes(u.to(DEV), 0.1)
    return (v.cpu().numpy().astype(np.float64) / (n - 1) * 2.0 - 1.0), f.cpu().numpy().astype(np.int64)


def check_depth(v, f, c2w, H, W, fx, fy, cx, cy, far=20.0):
    """Coverage identical away from projected edges (1e-3 px) and the near/far planes; depth to a relative 1e-5.
    Bound: the kernel computes the ray-plane intersection in fp64 from fp32 vertices / matrices (the same inputs the
    restatement widens exactly), then rounds once to fp32: |rel error| <= 2^-24 + O(1e-13) of fp64 evaluation, far below
    1e-5; the tolerance leaves room for the restatement's different (but also fp64) operation order."""
    from go_slam_amd.neus.mesher import render_mesh_depth
    v32 = np.asarray(v, np.float32)
    c2w32 = np.asarray(c2w, np.float32)
    got = render_mesh_depth((v32, f), torch.from_numpy(c2w32), H, W, fx, fy, cx, cy, far=far).cpu().numpy()
    ref, amb = CR.mesh_depth(v32.astype(np.float64), f, c2w32.astype(np.float64), H, W, fx, fy, cx, cy, far=far)
    ok = ~amb
    assert np.array_equal(got[ok] > 0, ref[ok] > 0), int(((got > 0) != (ref > 0))[ok].sum())
    both = ok & (ref > 0)
    assert np.all(np.abs(got[both] - ref[both]) <= 1e-5 * ref[both])
    again = render_mesh_depth((v32, f), torch.from_numpy(c2w32), H, W, fx, fy, cx, cy, far=far).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))
    return got, ref, amb


@pytest.mark.parametrize("H,W", [(48, 64), (240, 320)])
def test_depth_matches_restatement(built_lib, H, W):
    sv, sf = sphere(10, 1.0)
    bv, bf = blob_mesh(1, 16)
    v = np.concatenate([sv * 0.4 + [0.3, 0.2, 0.1], bv])
    f = np.concatenate([sf, bf + len(sv)])
    poses = [look_at((3.0, 0.5, 0.7), (0, 0, 0)), look_at((-0.2, 2.6, -1.1), (0.1, 0, 0)),
             look_at((0.05, 0.1, 0.02), (1, 0.3, 0.2)), look_at((0.3, -0.2, 0.1), (-1, -0.2, 0.4))]  # last two inside
    fx = fy = 0.8 * W
    got, ref, amb = check_depth(v, f, np.stack(poses), H, W, fx, fy, W / 2 - 0.3, H / 2 + 0.2)
    assert (ref > 0).mean() > 0.2 and amb.mean() < 0.05


def test_closed_sphere_is_watertight(built_lib):
    from go_slam_amd.neus.mesher import render_mesh_depth
    H = W = 96
    f = 90.0
    v, fc = sphere(96, 1.0)
    c2w = np.eye(4)
    c2w[2, 3] = -3.0
    d = render_mesh_depth((v, fc), torch.from_numpy(c2w[None]), H, W, f, f, W / 2, H / 2).cpu().numpy()[0]
    # silhouette of the inscribed polyhedron: the sphere's, shrunk; one pixel inward of the analytic silhouette radius
    r_px = f * 1.0 / np.sqrt(3.0 ** 2 - 1.0) * np.cos(np.pi / 96)
    X, Y = np.meshgrid(np.arange(W) + 0.5 - W / 2, np.arange(H) + 0.5 - H / 2)
    inner = np.hypot(X, Y) < r_px - 1.0
    assert inner.sum() > 2500 and (d[inner] > 0).all()


def test_special_triangles(built_lib):
    H, W, fx, fy, cx, cy = 48, 64, 50.0, 50.0, 32.0, 24.0
    eye = np.eye(4)[None]
    # covering the whole image
    v = np.array([[-1e3, -1e3, 2.0], [1e3, -1e3, 2.0], [0.0, 1e3, 2.0]])
    got, ref, _ = check_depth(v, np.array([[0, 1, 2]]), eye, H, W, fx, fy, cx, cy)
    assert (got > 0).all() and np.allclose(got, 2.0)
    # straddling znear: its front part renders
    v = np.array([[-2.0, -2.0, -1.0], [2.0, -2.0, -1.0], [0.0, 2.0, 3.0]])
    got, ref, _ = check_depth(v, np.array([[0, 1, 2]]), eye, H, W, fx, fy, cx, cy)
    assert 0 < (got > 0).sum() < H * W
    # behind the camera, beyond far: nothing
    v = np.array([[-1.0, -1.0, -2.0], [1.0, -1.0, -2.0], [0.0, 1.0, -2.0], [-1, -1, 30.0], [1, -1, 30.0], [0, 1, 30.0]])
    got, _, _ = check_depth(v, np.array([[0, 1, 2], [3, 4, 5], [0, 0, 1]]), eye, H, W, fx, fy, cx, cy)
    assert not got.any()


def test_chunked_equals_per_pose(built_lib):
    from go_slam_amd.neus.mesher import render_mesh_depth
    v, f = blob_mesh(2, 20)
    g = np.random.default_rng(4)
    poses = np.stack([look_at(g.normal(size=3) * 2.5, g.normal(size=3) * 0.2) for _ in range(300)])
    H, W = 48, 64
    all_ = render_mesh_depth((v, f), torch.from_numpy(poses), H, W, 50, 50, 32, 24, chunk=128).cpu().numpy()
    for k in range(0, 300, 37):
        one = render_mesh_depth((v, f), torch.from_numpy(poses[k:k + 1]), H, W, 50, 50, 32, 24).cpu().numpy()
        assert np.array_equal(all_[k].view(np.uint32), one[0].view(np.uint32))
    assert (all_ > 0).mean() > 0.05


@pytest.mark.parametrize("radius", [0.0, 25.0, -5.0])
def test_point_masks_match_restatement(built_lib, radius):
    from go_slam_amd.neus.mesher import point_masks, render_mesh_depth
    v, f = blob_mesh(3, 24)
    g = np.random.default_rng(5)
    poses = np.stack([look_at(g.normal(size=3) * 0.3, g.normal(size=3)) for _ in range(12)]
                     + [look_at(g.normal(size=3) * 2.5, g.normal(size=3) * 0.1) for _ in range(12)])
    H, W, fx, fy, cx, cy = 48, 64, 40.0, 41.0, 31.5, 23.7
    depth = render_mesh_depth((v, f), torch.from_numpy(poses), H, W, fx, fy, cx, cy)
    seen, fc = point_masks(v, depth, torch.from_numpy(poses), H, W, fx, fy, cx, cy, radius, chunk=7)
    rs, rf, margin = CR.point_masks(v, depth.cpu().numpy(), poses, H, W, fx, fy, cx, cy, radius)
    delta = 1e-4
    sure = margin > delta
    assert sure.mean() > 0.98
    assert np.array_equal(seen.cpu().numpy()[sure], rs[sure]) and np.array_equal(fc.cpu().numpy()[sure], rf[sure])
    assert rs.sum() > 50 and (~rs).sum() > 50                                # both outcomes occur


def room_mesh():
    """Marching cubes of an analytic room: walls of a box, a table, a pillar and floating specks."""
    from go_slam_amd.neus.mesh import marching_cubes
    n = 64
    x = np.linspace(-2.0, 2.0, n)
    X, Y, Z = np.meshgrid(x, x, x, indexing="ij")
    room = 1.8 - np.max(np.abs(np.stack([X, Y, Z * 1.2])), axis=0)
    table = np.maximum.reduce([np.abs(X - 0.5) - 0.5, np.abs(Y + 0.3) - 0.35, np.abs(Z + 0.6) - 0.05])
    pillar = np.hypot(X + 0.9, Y - 0.8) - 0.15
    speck = np.min([np.sqrt((X - a) ** 2 + (Y - b) ** 2 + (Z - c) ** 2) - 0.07
                    for a, b, c in [(0.2, 0.9, 0.8), (-0.7, -0.6, 0.3), (1.0, 0.1, -0.2)]], axis=0)
    sdf = np.minimum.reduce([room, table, pillar, speck])
    v, f = marching_cubes(torch.from_numpy(-sdf.astype(np.float32)).to(DEV), 0.0)
    return v.cpu().numpy().astype(np.float64) / (n - 1) * 4.0 - 2.0, f.cpu().numpy().astype(np.int64)


def test_components_match_restatement(built_lib):
    from go_slam_amd.neus.mesher import face_components
    cases = [room_mesh(), blob_mesh(6, 30)]
    g = np.random.default_rng(7)
    soup_f = g.integers(0, 400, size=(3000, 3))
    soup_f[:50, 1] = soup_f[:50, 0]                                         # degenerate edges
    soup_f[100:160] = soup_f[100]                                           # repeated faces: non-manifold edges
    cases.append((g.random((400, 3)), soup_f))
    for v, f in cases:
        labels, comp_area, total = face_components(f, v)
        rl, ra, rt = CR.face_components(f, v)
        assert np.array_equal(labels.cpu().numpy(), rl)
        ca = comp_area.cpu().numpy()
        roots = np.array(sorted(ra))
        assert np.allclose(ca[roots], [ra[r] for r in roots], rtol=1e-12, atol=0)
        assert np.count_nonzero(ca) <= len(roots) and abs(total - rt) <= 1e-12 * rt
        l2, a2, t2 = face_components(f, v)
        assert torch.equal(labels, l2) and torch.equal(comp_area, a2) and t2 == total
    assert len(np.unique(CR.face_components(cases[0][1]))) >= 5


def test_components_at_3m_faces(built_lib):
    from go_slam_amd.neus.mesh import marching_cubes
    from go_slam_amd.neus.mesher import face_components
    g = torch.Generator().manual_seed(8)
    u = torch.nn.functional.interpolate(torch.randn(1, 1, 24, 24, 24, generator=g), size=(256, 256, 256),
                                        mode="trilinear", align_corners=True)[0, 0]
    v, f = marching_cubes(u.to(DEV), 0.0)
    assert f.shape[0] > 2_000_000
    labels, comp_area, total = face_components(f, v.double())
    rl = CR.face_components(f.cpu().numpy())
    assert np.array_equal(labels.cpu().numpy(), rl)


def hull_vertex_set(p):
    from scipy.spatial import ConvexHull
    p = np.asarray(p, np.float64)
    return {tuple(x) for x in p[ConvexHull(p).vertices]}


def test_hull_prefilter_keeps_every_hull_vertex(built_lib):
    from go_slam_amd.neus.mesher import hull_candidates
    g = np.random.default_rng(9)
    cube = g.random((20000, 3)) - 0.5
    ax = g.integers(0, 3, 20000)
    cube[np.arange(20000), ax] = np.sign(cube[np.arange(20000), ax]) * 0.5            # on the cube's surface
    slab = g.normal(size=(20000, 3)) * [3.0, 2.0, 1e-4]
    clouds = [g.normal(size=(50000, 3)), g.random((50000, 3)) * [5, 1, 0.2] + 3.0, cube, slab,
              np.concatenate([g.normal(size=(30000, 3)) * 0.1, np.array([[5.0, 5, 5], [-5, 5, 5]])])]
    for c in clouds:
        c32 = c.astype(np.float32)
        surv, mask = hull_candidates(torch.from_numpy(c32).to(DEV))
        if c is not cube and c is not slab:      # every point of a cube's surface lies on the extremes' hull
            assert surv.shape[0] < len(c) // 2
        assert hull_vertex_set(surv.cpu().numpy()) == hull_vertex_set(c32)


def test_obb_matches_restatement(built_lib):
    from go_slam_amd.neus.mesher import OrientedBoundingBox
    g = np.random.default_rng(10)
    local = g.normal(size=(200000, 3)) * [2.0, 1.0, 0.4]
    a = 0.7
    R0 = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    pts = (local @ R0.T + [0.5, -1.0, 2.0]).astype(np.float32)
    for inp in (pts, torch.from_numpy(pts).to(DEV)):
        box = OrientedBoundingBox().to(DEV)
        box.compute_from_pointcloud(inp, extend=0.1)
        c, R, e = CR.obb(pts.astype(np.float64), extend=0.1)
        assert np.allclose(box.center.cpu().numpy(), c, atol=1e-9, rtol=0)
        assert np.allclose(box.extent.cpu().numpy(), e, atol=1e-9, rtol=0)
        assert box.survivors < len(pts) // 10
        q = g.normal(size=(50000, 3)) * 2.0
        got = box.in_bound(q)
        ref, dist = CR.obb_in_bound(q, c, R, e)
        away = dist > 1e-7
        assert isinstance(got, np.ndarray) and np.array_equal(got[away], ref[away])
        aabb = box.get_axis_aligned_bounding_box()
        assert aabb.shape == (3, 2) and aabb.dtype == np.float32


def _cfg(radius, largest):
    return {"meshing": {"resolution": 96, "level_set": 0.0, "remove_small_geometry_threshold": 0.2,
                        "get_largest_components": largest, "eval_rec": False, "n_points_to_eval": 1000,
                        "mesh_threshold_to_eval": 0.05, "gt_mesh_path": "/nonexistent/gt.ply", "forecast_radius": radius},
            "mapping": {"device": DEV}}


@pytest.mark.parametrize("radius,largest", [(0, False), (25, False), (0, True), (25, True)])
def test_cull_mesh_equals_host_composition(built_lib, tmp_path, radius, largest):
    from test_mesh_gpu import _model
    from go_slam_amd.neus.mesher import Mesher
    model, _ = _model()
    mesh = model.extract_geometry(40, 0.0, save_path=None)
    H, W, fx, fy, cx, cy = 48, 64, 40.0, 40.0, 32.0, 24.0
    g = np.random.default_rng(11)
    ctr = mesh.vertices.mean(0)
    poses = np.stack([look_at(ctr + g.normal(size=3) * 0.3, ctr + g.normal(size=3)) for _ in range(6)])
    slam = types.SimpleNamespace(output=str(tmp_path), mapping_net=model, video=None, reload_map=0, verbose=False,
                                 H=H, W=W, fx=fx, fy=fy, cx=cx, cy=cy)
    m = Mesher(_cfg(radius, largest), None, slam)
    bound = np.stack([mesh.vertices.min(0) + 0.2, mesh.vertices.max(0) - 0.1], 1)
    (cv, cf), (fv, ff) = CR.cull_mesh(mesh.vertices, mesh.faces, poses, bound, H, W, fx, fy, cx, cy, radius, 0.2, largest)
    out = str(tmp_path / "mesh" / "final_raw_mesh.ply")
    cull, fore = m.cull_mesh(mesh.copy(), torch.from_numpy(poses).float(), bound, out)
    assert len(cf) > 50
    assert np.array_equal(cull.faces, cf) and np.array_equal(cull.vertices, cv)
    assert np.array_equal(fore.faces, ff) and np.array_equal(fore.vertices, fv)
    for name in ("bound_mesh.ply", "mesh_with_hole.ply", "final_raw_mesh.ply", "final_raw_mesh_forecast.ply"):
        assert (tmp_path / "mesh" / name).exists(), name


def test_mesher_call_without_open3d_pyrender_trimesh(built_lib, tmp_path, monkeypatch):
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
    video = DepthVideo(6, 8, buffer=8, device=DEV, full_res=True)           # 48 x 64 full resolution
    n = 5
    yy, xx = torch.meshgrid(torch.arange(48.0), torch.arange(64.0), indexing="ij")
    bump = 0.5 + 0.1 * torch.sin(xx / 9.0) * torch.cos(yy / 7.0)              # a curved surface: a 3-D cloud
    for i in range(n):
        video.poses[i] = torch.tensor([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0])
        video.disps_up[i] = bump
        video.timestamp[i] = float(i)
    video.intrinsics[:n] = torch.tensor([5.0, 5.0, 4.0, 3.0])
    video.counter.value = n
    slam = types.SimpleNamespace(output=str(tmp_path), mapping_net=model, video=video,
                                 reload_map=torch.zeros(1).int(), verbose=False, H=48, W=64, fx=40.0, fy=40.0,
                                 cx=32.0, cy=24.0)
    m = Mesher(_cfg(25, False), None, slam)
    m(the_end=True)
    assert (tmp_path / "mesh" / "final_raw_mesh.ply").exists()
    assert (tmp_path / "mesh" / "mesh_with_hole.ply").exists()
    assert int(m.reload_map) == -1
