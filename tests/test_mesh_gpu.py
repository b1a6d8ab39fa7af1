"""Mesh extraction on the MI355X: the HIP marching cubes equals the serial restatement (tests/mesh_restatement.py) bit
for bit, the 64-bit totals and offsets hold at 1024^3, the fused SDF lattice matches extract_fields and the oracle, and
InstantNeuS.extract_geometry equals the same steps composed on the host."""
import numpy as np
import pytest
import torch

import mesh_restatement as MR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def assert_same_mesh(got, ref):
    (gv, gf), (rv, rf) = got, ref
    gv, gf = gv.cpu().numpy(), gf.cpu().numpy()
    assert gv.dtype == np.float32 and gf.dtype == np.int32
    assert gv.shape == rv.shape and gf.shape == rf.shape
    nan = np.isnan(rv)
    assert np.array_equal(np.isnan(gv), nan)
    assert np.array_equal(gv.view(np.uint32)[~nan], rv.view(np.uint32)[~nan])        # bit for bit
    assert np.array_equal(gf, rf)


def mc_both(u, level=0.0):
    from go_slam_amd.neus.mesh import marching_cubes
    u = np.ascontiguousarray(u, dtype=np.float32)
    got = marching_cubes(torch.from_numpy(u).to(DEV), level)
    assert_same_mesh(got, MR.marching_cubes(u, level))
    return got


def smooth_field(shape, seed, coarse=(6, 5, 7)):
    g = torch.Generator().manual_seed(seed)
    n = torch.randn((1, 1) + coarse, generator=g)
    return torch.nn.functional.interpolate(n, size=shape, mode="trilinear", align_corners=True)[0, 0].numpy()


def lattice(shape):
    return np.meshgrid(*[np.arange(s, dtype=np.float64) for s in shape], indexing="ij")


def test_sphere_and_torus_match_restatement(built_lib):
    x, y, z = lattice((30, 31, 30))
    mc_both((12.0 - np.sqrt((x - 14.3) ** 2 + (y - 15.1) ** 2 + (z - 14.7) ** 2)).astype(np.float32))
    x, y, z = lattice((33, 32, 22))
    q = np.sqrt((x - 16.2) ** 2 + (y - 15.7) ** 2) - 10.0
    mc_both((4.0 - np.sqrt(q ** 2 + (z - 10.4) ** 2)).astype(np.float32), 0.25)


@pytest.mark.parametrize("shape", [(33, 29, 31), (64, 64, 64), (17, 40, 9), (3, 200, 5), (130, 7, 70)])
def test_random_fields_match_restatement(built_lib, shape):
    for k, coarse in enumerate([(6, 5, 7), (12, 11, 13)]):
        mc_both(smooth_field(shape, 11 + k, coarse), 0.03 * k)
    g = np.random.default_rng(5)
    mc_both(g.standard_normal(shape).astype(np.float32), -0.1)           # every case, every ambiguous face


def test_numpy_input_is_uploaded(built_lib):
    from go_slam_amd.neus.mesh import marching_cubes
    u = smooth_field((20, 21, 22), 3)
    got = marching_cubes(u, 0.0)
    assert got[0].is_cuda and got[1].is_cuda
    assert_same_mesh(got, MR.marching_cubes(u, 0.0))


def test_corners_exactly_at_level_and_nan_corners(built_lib):
    g = np.random.default_rng(9)
    u = (np.round(smooth_field((29, 31, 27), 4, (7, 6, 5)) * 2.0) / 2.0).astype(np.float32)   # many exact zeros
    assert (u == 0).mean() > 0.2
    mc_both(u, 0.0)
    mc_both(u, 0.5)
    v = smooth_field((25, 26, 27), 6)
    v[g.random(v.shape) < 0.05] = np.nan
    assert np.isnan(v).any()
    got = mc_both(v, 0.0)
    assert bool(torch.isnan(got[0]).any())


def test_thin_and_tiny_volumes(built_lib):
    g = np.random.default_rng(2)
    for shape in [(1, 40, 40), (40, 1, 40), (40, 40, 1), (1, 1, 50), (1, 1, 1), (2, 2, 2), (2, 3, 2)]:
        mc_both(g.standard_normal(shape).astype(np.float32))
    # every one of the 256 cases on its own cube
    for case in range(256):
        u = np.array([1.0 if (case >> c) & 1 else -1.0 for c in range(8)], np.float32)
        vol = np.zeros((2, 2, 2), np.float32)
        for c, (dx, dy, dz) in enumerate(MR.CORNERS):
            vol[dx, dy, dz] = -u[c] * (0.5 + 0.06 * c)                    # corner c below iff bit c set
        v, f = mc_both(vol)
        assert len(f) == len(MR.TRI_TABLE[case]) // 3


def test_empty_surfaces(built_lib):
    from go_slam_amd.neus.mesh import marching_cubes
    for u in [np.full((9, 10, 11), 2.0, np.float32), np.full((9, 10, 11), -2.0, np.float32),
              np.full((9, 10, 11), np.nan, np.float32), np.zeros((1, 1, 1), np.float32)]:
        v, f = marching_cubes(torch.from_numpy(u).to(DEV), 0.0)
        assert v.shape == (0, 3) and f.shape == (0, 3) and v.is_cuda and f.is_cuda


def test_emit_refuses_int32_overflow(built_lib):
    """gs_mcubes_emit returns GS_ERR_UNSUPPORTED for totals beyond INT32_MAX and launches nothing."""
    from go_slam_amd import _lib
    L = _lib.lib()
    u = torch.zeros(2, 2, 2, device=DEV)
    ws = torch.empty(L.gs_mcubes_workspace_bytes(2, 2, 2), dtype=torch.uint8, device=DEV)
    out = torch.full((4, 3), 7.0, device=DEV)
    rc = L.gs_mcubes_emit(_lib.ptr(u), 2, 2, 2, 0.0, _lib.ptr(ws), ws.numel(), 2 ** 31, 1, _lib.ptr(out),
                          _lib.ptr(out), _lib.stream_ptr(None))
    assert rc == -4
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


def test_plane_at_1024_cubed(built_lib):
    """u = x - 511.3 on the largest supported lattice (4 GB): V = r^2, F = 2 (r-1)^2, every vertex at the expected x.
    Exercises the 64-bit totals, the chunk prefix and point indices near 2^30.  A checkerboard on the same lattice has
    more than 2^31 vertices and must be refused before anything is allocated for it."""
    from go_slam_amd.neus.mesh import marching_cubes
    r = 1024
    col = torch.arange(r, dtype=torch.float32, device=DEV) - 511.3
    u = col.view(r, 1, 1).expand(r, r, r).contiguous()
    v, f = marching_cubes(u, 0.0)
    assert v.shape == (r * r, 3) and f.shape == (2 * (r - 1) ** 2, 3)
    u0, u1 = (np.float32(x) for x in u[511:513, 0, 0].cpu().numpy())
    t = (np.float32(0.0) - u0) / (u1 - u0)
    x_expected = np.float32(511.0) + t * (np.float32(512.0) - np.float32(511.0))
    vc = v.cpu().numpy()
    assert np.array_equal(vc[:, 0], np.full(r * r, x_expected, np.float32))
    jj, kk = np.meshgrid(np.arange(r, dtype=np.float32), np.arange(r, dtype=np.float32), indexing="ij")
    assert np.array_equal(vc[:, 1], jj.reshape(-1)) and np.array_equal(vc[:, 2], kk.reshape(-1))
    fc = f.cpu().numpy().astype(np.int64)
    assert fc.min() == 0 and fc.max() == r * r - 1
    n = np.cross(vc[fc[:, 1]] - vc[fc[:, 0]], vc[fc[:, 2]] - vc[fc[:, 0]])
    assert (n[:, 0] < 0).all()                                           # toward decreasing u
    del v, f, vc, fc, n
    ii = torch.arange(r, device=DEV, dtype=torch.int32)
    parity = (ii.view(r, 1, 1) + ii.view(1, r, 1) + ii.view(1, 1, r)) & 1
    u.copy_(parity.float() * 2.0 - 1.0)
    del parity
    with pytest.raises(RuntimeError, match="exceed int32"):
        marching_cubes(u, 0.0)


# ---- the fused SDF lattice
def _model(seed=83, rt=((-1.0, 1.5), (-1.0, 2.0), (-0.5, 2.0))):
    import go_slam_amd.neus as N
    from oracle import neus_oracle as O
    P = O.make_params(seed, grid_init=0.2, bound=((-2.0, 2.0), (-1.5, 2.5), (-1.0, 3.0)))
    model = N.InstantNeuS({}, P["bound"].tolist(), device=DEV).to(DEV)
    with torch.no_grad():
        model.sdf_network.encoding.encoding.params.copy_(P["grid"])
        model.sdf_network.sdf_layer.weight.copy_(P["sdf_w"])
        model.sdf_network.sdf_layer.bias.copy_(P["sdf_b"] + 0.05)
        model.color_network._B.copy_(P["color_B"])
        model.color_network.network.params.copy_(P["mlp"])
    if rt is not None:
        model.update_bound(torch.tensor(rt))
    return model, P


@pytest.mark.parametrize("res", [21, 96])
def test_sdf_lattice_matches_extract_fields(built_lib, res):
    """Same -100 mask exactly.  Inside, both sides dot the same fp16 features and the same normalised point with W0
    (35 terms) and add the bias; only the summation order differs (the kernel: one fmaf chain; extract_fields: a library
    GEMM, order unknown).  Each evaluation of a sum of n = 36 terms t_i in fp32, in any order, is within
    gamma_n sum |t_i| of the exact sum (gamma_n = n u / (1 - n u), u = 2^-24), so the two differ by at most
    2 gamma_36 sum |t_i|; that bound, computed per point in float64, is the tolerance."""
    model, P = _model()
    u = model.sdf_lattice(model.bound[:, 0], model.bound[:, 1], res)
    assert u.is_cuda and u.dtype == torch.float32 and u.shape == (res, res, res)
    ref = torch.from_numpy(model.extract_fields(model.bound[:, 0], model.bound[:, 1], res))
    got = u.cpu()
    out = ref == -100.0
    assert torch.equal(got == -100.0, out) and 0 < int(out.sum()) < out.numel()
    lin = [torch.linspace(float(P["bound"][k, 0]), float(P["bound"][k, 1]), res, device=DEV) for k in range(3)]
    xx, yy, zz = torch.meshgrid(*lin, indexing="ij")
    pts = torch.stack([xx.reshape(-1), yy.reshape(-1), zz.reshape(-1)], 1)[~out.reshape(-1).to(DEV)]
    b = model.bound
    p = ((pts - b[:, 0]) / (b[:, 1] - b[:, 0]) * 2.0 - 1.0).clamp(-1.0, 1.0)
    with torch.no_grad():
        enc = model.sdf_network.encoding.encoding((p + 1) / 2)
    x = torch.cat([p, enc.float()], 1).double()
    w0 = model.sdf_network.sdf_layer.weight[0].double()
    mag = (x * w0).abs().sum(1) + model.sdf_network.sdf_layer.bias[0].double().abs()
    n, unit = 36, 2.0 ** -24
    tol = 2.0 * (n * unit / (1 - n * unit)) * mag
    diff = (got[~out].double().to(DEV) - ref[~out].double().to(DEV)).abs()
    assert bool((diff <= tol).all()), float((diff / tol).max())


def test_sdf_lattice_matches_oracle(built_lib):
    """against oracle.neus_oracle.sdf_and_gradient at test_widen_gpu.py's point-query tolerances"""
    from oracle import neus_oracle as O
    model, P = _model(rt=None)
    res = 17
    u = model.sdf_lattice(model.bound[:, 0], model.bound[:, 1], res).cpu()
    lin = [torch.linspace(float(P["bound"][k, 0]), float(P["bound"][k, 1]), res) for k in range(3)]
    xx, yy, zz = torch.meshgrid(*lin, indexing="ij")
    pts = torch.stack([xx.reshape(-1), yy.reshape(-1), zz.reshape(-1)], 1)
    inside = ((pts > P["bound"][:, 0]) & (pts < P["bound"][:, 1])).all(1)
    sdf_r, _, _ = O.sdf_and_gradient(pts, P["bound"], P["grid"], P["sdf_w"], P["sdf_b"] + 0.05)
    ref = torch.where(inside, -sdf_r[:, 0], torch.full_like(sdf_r[:, 0], -100.0))
    torch.testing.assert_close(u.reshape(-1), ref, rtol=1e-4, atol=2e-5)


# ---- extract_geometry end to end
def _host_composition(model, res, threshold, c2w_ref, color):
    u = model.sdf_lattice(model.bound[:, 0], model.bound[:, 1], res).cpu().numpy()
    v, f = MR.marching_cubes(u, threshold)
    b = model.bound.cpu().numpy()
    verts = v.astype(np.float64) / (res - 1.0) * (b[:, 1] - b[:, 0])[None, :] + b[:, 0][None, :]
    if c2w_ref is not None:
        c2w = c2w_ref.cpu().numpy().astype(np.float64)
        vh = np.concatenate([verts, np.ones_like(verts[:, :1])], axis=1)
        verts = np.matmul(c2w[None], vh[:, :, None])[:, :3, 0]
    rt = model.realtime_bound.cpu().numpy()
    keep_v = np.all(verts >= rt[:, 0] - 0.01, axis=1) & np.all(verts <= rt[:, 1] + 0.01, axis=1)
    faces = f.astype(np.int64)[keep_v[f].all(axis=1)]
    used = np.unique(faces)                                   # ascending = the original relative order
    remap = np.full(len(verts), -1, np.int64)
    remap[used] = np.arange(len(used))
    verts, faces = verts[used], remap[faces]
    cols = model.extract_color(model.bound.clone(), verts) if color else None
    return verts, faces, cols


@pytest.mark.parametrize("with_c2w", [False, True])
def test_extract_geometry_equals_host_composition(built_lib, tmp_path, with_c2w):
    model, _ = _model()
    res, thr = 48, 0.0
    c2w = None
    if with_c2w:
        a = 0.3
        c2w = torch.tensor([[np.cos(a), -np.sin(a), 0.0, 0.2], [np.sin(a), np.cos(a), 0.0, -0.1],
                            [0.0, 0.0, 1.0, 0.05], [0.0, 0.0, 0.0, 1.0]], dtype=torch.float32)
    path = str(tmp_path / "mesh.ply")
    mesh = model.extract_geometry(res, thr, c2w_ref=c2w, save_path=path, color=True)
    rv, rf, rc = _host_composition(model, res, thr, c2w, True)
    assert len(rf) > 100
    if with_c2w:                                              # the rotation takes part of the surface out of the bound
        assert len(rv) < len(MR.marching_cubes(model.sdf_lattice(model.bound[:, 0], model.bound[:, 1], res).cpu().numpy(),
                                               thr)[0])
    assert mesh.vertices.dtype == np.float64 and mesh.faces.dtype == np.int64 and mesh.vertex_colors.dtype == np.uint8
    assert np.array_equal(mesh.vertices, rv) and np.array_equal(mesh.faces, rf)
    assert np.array_equal(mesh.vertex_colors, rc)
    pv, pf, pc = MR.read_ply(path)
    assert np.array_equal(pv, rv) and np.array_equal(pf, rf) and np.array_equal(pc, rc)
    plain = model.extract_geometry(res, thr, c2w_ref=c2w, save_path=None, color=False)
    assert plain.vertex_colors is None
    assert np.array_equal(plain.vertices, rv) and np.array_equal(plain.faces, rf)


def test_extract_geometry_default_signature(built_lib, tmp_path, monkeypatch):
    """the reference's defaults: c2w_ref=None, save_path='./mesh.ply', color=False"""
    model, _ = _model()
    monkeypatch.chdir(tmp_path)
    mesh = model.extract_geometry(32, 0.0)
    assert (tmp_path / "mesh.ply").exists() and mesh.vertex_colors is None
    pv, pf, pc = MR.read_ply(str(tmp_path / "mesh.ply"))
    assert np.array_equal(pv, mesh.vertices) and np.array_equal(pf, mesh.faces) and pc is None
