"""Mesh extraction without a GPU: the new entry points are declared and exported, the serial restatement of the
marching-cubes contract (tests/mesh_restatement.py, what the HIP kernels must equal bit for bit) produces watertight,
correctly wound, crack-free meshes, and Mesh.export writes a PLY that parses back."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import mesh_restatement as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ["gs_sdf_lattice", "gs_mcubes_workspace_bytes", "gs_mcubes_count", "gs_mcubes_scan", "gs_mcubes_emit"]


def test_mesh_entries_declared_and_exported(built_lib):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "goslam_neus.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gs_[a-z0-9_]+)\s*\(", src))
    handle = ctypes.CDLL(built_lib)
    for name in NEW_ENTRIES:
        assert name in declared, name
        assert hasattr(handle, name), name
    from go_slam_amd import _lib
    assert set(NEW_ENTRIES) <= set(_lib.SIGNATURES)


def test_workspace_query(built_lib):
    from go_slam_amd import _lib
    L = _lib.lib()
    assert L.gs_mcubes_workspace_bytes(512, 512, 512) == 272642048          # the figures include/goslam_neus.h states
    assert L.gs_mcubes_workspace_bytes(1024, 1024, 1024) == 2181136384
    assert L.gs_mcubes_workspace_bytes(1, 1, 1) > 0
    assert L.gs_mcubes_workspace_bytes(0, 4, 4) == 0 and L.gs_mcubes_workspace_bytes(1025, 4, 4) == 0


# ---- topology helpers
def mesh_edges(f):
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    return np.unique(e, axis=0, return_counts=True)


def components(n_vertices, f):
    parent = np.arange(n_vertices)

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for a, b in np.concatenate([f[:, [0, 1]], f[:, [1, 2]]]):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[ra] = rb
    used = np.unique(f)
    return len({find(a) for a in used})


def signed_volume(v, f):
    a, b, c = (v[f[:, k]].astype(np.float64) for k in range(3))
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def lattice(shape):
    return np.meshgrid(*[np.arange(s, dtype=np.float64) for s in shape], indexing="ij")


def smooth_field(shape, seed, coarse=(6, 5, 7)):
    g = torch.Generator().manual_seed(seed)
    n = torch.randn((1, 1) + coarse, generator=g)
    return torch.nn.functional.interpolate(n, size=shape, mode="trilinear", align_corners=True)[0, 0].numpy()


# ---- restatement on analytic fields
def test_sphere_watertight_wound_outward():
    R, c = 12.0, np.array([14.3, 15.1, 14.7])
    x, y, z = lattice((30, 31, 30))
    d = np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2)
    u = (R - d).astype(np.float32)                         # u = -sdf: below = outside, normals point out of the solid
    v, f = MR.marching_cubes(u, 0.0)
    assert v.dtype == np.float32 and f.dtype == np.int32 and len(f) > 1000
    _, cnt = mesh_edges(f)
    assert (cnt == 2).all()                                # watertight
    V, E, F = len(v), len(cnt), len(f)
    assert V - E + F == 2
    assert components(V, f) == 1
    r = np.linalg.norm(v.astype(np.float64) - c, axis=1)
    assert np.abs(r - R).max() < 0.05
    vol = signed_volume(v, f)
    assert vol > 0 and abs(vol / (4.0 / 3.0 * np.pi * R ** 3) - 1.0) < 0.01


def test_torus_euler_zero():
    c = np.array([16.2, 15.7, 10.4])
    x, y, z = lattice((33, 32, 22))
    q = np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2) - 10.0
    u = (4.0 - np.sqrt(q ** 2 + (z - c[2]) ** 2)).astype(np.float32)
    v, f = MR.marching_cubes(u, 0.0)
    _, cnt = mesh_edges(f)
    assert (cnt == 2).all()
    assert len(v) - len(cnt) + len(f) == 0
    assert components(len(v), f) == 1
    assert signed_volume(v, f) > 0


@pytest.mark.parametrize("shape,seed", [((33, 29, 31), 0), ((33, 29, 31), 1), ((17, 40, 9), 2), ((25, 25, 25), 3),
                                        ((12, 13, 14), 4)])
def test_random_fields_have_no_cracks(shape, seed):
    """Every mesh edge that does not lie on the volume's outer faces is shared by exactly two faces: neighbouring cubes
    resolve their shared (possibly ambiguous) face the same way."""
    for k, u in enumerate([smooth_field(shape, seed), smooth_field(shape, seed + 100, coarse=(12, 11, 13))]):
        v, f = MR.marching_cubes(u, 0.05 * k)
        e, cnt = mesh_edges(f)
        ve = v[e]                                          # [E, 2, 3]
        hi = np.array(shape, dtype=np.float32) - 1
        outer = np.zeros(len(e), dtype=bool)
        for d in range(3):
            for s in (0.0, hi[d]):
                outer |= (ve[:, 0, d] == s) & (ve[:, 1, d] == s)
        assert len(f) > 100
        assert (cnt[~outer] == 2).all(), (shape, seed, int((cnt[~outer] != 2).sum()))
        assert (cnt <= 2).all()


def test_every_case_closes_on_white_noise():
    """Per-voxel noise reaches every case and every ambiguous face; interior edges are still shared by two faces."""
    g = np.random.default_rng(7)
    for _ in range(10):
        u = g.standard_normal((11, 12, 13)).astype(np.float32)
        v, f = MR.marching_cubes(u, 0.0)
        e, cnt = mesh_edges(f)
        ve = v[e]
        hi = np.array(u.shape, dtype=np.float32) - 1
        outer = np.zeros(len(e), dtype=bool)
        for d in range(3):
            for s in (0.0, hi[d]):
                outer |= (ve[:, 0, d] == s) & (ve[:, 1, d] == s)
        assert (cnt[~outer] == 2).all()


def test_table_shape():
    assert len(MR.TRI_TABLE) == 256
    assert MR.TRI_TABLE[0] == () and MR.TRI_TABLE[255] == ()
    assert all(len(t) % 3 == 0 and len(t) <= 15 for t in MR.TRI_TABLE)
    # complementary single-corner cases wind oppositely
    assert sorted(MR.TRI_TABLE[1]) == sorted(MR.TRI_TABLE[254])
    assert MR.TRI_TABLE[1] != MR.TRI_TABLE[254]


def test_degenerate_volumes():
    v, f = MR.marching_cubes(np.ones((4, 5, 6), np.float32), 0.0)
    assert v.shape == (0, 3) and f.shape == (0, 3)
    v, f = MR.marching_cubes(-np.ones((4, 5, 6), np.float32), 0.0)
    assert v.shape == (0, 3) and f.shape == (0, 3)
    u = np.arange(9, dtype=np.float32).reshape(1, 3, 3) - 3.5      # no cube: vertices, no faces
    v, f = MR.marching_cubes(u, 0.0)
    assert len(v) == 4 and len(f) == 0
    assert np.array_equal(v[:, 0], np.zeros(4, np.float32))


# ---- PLY export
@pytest.mark.parametrize("coloured", [False, True])
def test_ply_export_round_trip(tmp_path, coloured):
    from go_slam_amd.neus.mesh import Mesh
    g = np.random.default_rng(3)
    V, F = 57, 91
    verts = g.standard_normal((V, 3))
    faces = g.integers(0, V, size=(F, 3))
    cols = g.integers(0, 256, size=(V, 3)).astype(np.uint8) if coloured else None
    m = Mesh(verts, faces, cols)
    path = str(tmp_path / "m.ply")
    assert m.export(path) == path
    rv, rf, rc = MR.read_ply(path)
    assert np.array_equal(rv, verts) and rv.dtype == np.float64
    assert np.array_equal(rf, faces)
    if coloured:
        assert np.array_equal(rc, cols)
    else:
        assert rc is None
    empty = Mesh(np.zeros((0, 3)), np.zeros((0, 3), np.int64))
    empty.export(path)
    rv, rf, rc = MR.read_ply(path)
    assert rv.shape == (0, 3) and rf.shape == (0, 3) and rc is None
