"""Mesh evaluation without a GPU: the NumPy restatement (tests/mesh_eval_restatement.py) against scipy and analytic
cases, the PLY reader, Mesh.apply_transform, the metrics file and the new entries' declarations."""
import ctypes
import os
import re

import numpy as np
import pytest

import mesh_eval_restatement as ER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ["gs_nn_cell_keys", "gs_nn_grid_build", "gs_nn_query_workspace_bytes", "gs_nn_query",
               "gs_icp_moments_workspace_bytes", "gs_icp_moments"]


def test_nn_entries_declared_and_exported(built_lib):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "goslam_neus.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gs_[a-z0-9_]+)\s*\(", src))
    handle = ctypes.CDLL(built_lib)
    from go_slam_amd import _lib
    for name in NEW_ENTRIES:
        assert name in declared and hasattr(handle, name) and name in _lib.SIGNATURES, name


def room(res=28):
    """Marching cubes (the serial restatement) of a box room with a table, vertices in metres."""
    import mesh_restatement as MR
    x = np.linspace(-1.5, 1.5, res)
    X, Y, Z = np.meshgrid(x, x, x, indexing="ij")
    walls = 1.3 - np.maximum(np.maximum(np.abs(X), np.abs(Y)), np.abs(Z * 1.2))
    table = np.maximum(np.maximum(np.abs(X - 0.3) - 0.4, np.abs(Y + 0.2) - 0.3), np.abs(Z + 0.5) - 0.08)
    v, f = MR.marching_cubes((-np.minimum(walls, table)).astype(np.float32), 0.0)
    return np.asarray(v, dtype=np.float64) / (res - 1) * 3.0 - 1.5, np.asarray(f, dtype=np.int64)


def rigid(deg, axis, t):
    from scipy.spatial.transform import Rotation
    T = np.eye(4)
    T[:3, :3] = Rotation.from_rotvec(np.deg2rad(deg) * np.asarray(axis) / np.linalg.norm(axis)).as_matrix()
    T[:3, 3] = t
    return T


def test_restated_nn_matches_ckdtree():
    from scipy.spatial import cKDTree
    g = np.random.default_rng(0)
    r = g.uniform(-1, 1, (3000, 3))
    q = g.uniform(-1.2, 1.2, (1500, 3))
    d2, idx = ER.nn(q, r)
    dist, j = cKDTree(r).query(q)
    np.testing.assert_allclose(np.sqrt(d2), dist, rtol=1e-12, atol=0)
    d_sorted = np.sort(((q[:, None] - r[None]) ** 2).sum(-1), axis=1)
    no_tie = d_sorted[:, 1] - d_sorted[:, 0] > 1e-12
    assert no_tie.mean() > 0.99 and np.array_equal(idx[no_tie], j[no_tie])


def test_restated_nn_ties_radius_and_transform():
    r = np.array([[0.0, 0, 0], [1.0, 0, 0], [1.0, 0, 0], [0.5, 0, 0]])
    d2, idx = ER.nn([[0.75, 0, 0], [1.0, 0, 0], [0.25, 0, 0]], r)
    assert list(idx) == [1, 1, 0]                 # equal d2: the smallest index
    d2, idx = ER.nn([[0.0, 0.0, 0.5]], r, max_distance=0.5)
    assert idx[0] == -1 and np.isinf(d2[0])       # exactly at the radius: outside (d2 < r^2)
    d2, idx = ER.nn([[0.0, 0.0, 0.49]], r, max_distance=0.5)
    assert idx[0] == 0
    T = rigid(90, (0, 0, 1), (1.0, 0, 0))
    d2, idx = ER.nn([[0.0, 0.5, 0.0]], r, transform=T)   # -> (0.5, 0, 0)
    assert idx[0] == 3 and d2[0] < 1e-30


@pytest.fixture(scope="module")
def room_mesh():
    return room()


def test_restated_icp_recovers_rigid_motion(room_mesh):
    v, _ = room_mesh
    T_true = rigid(3.0, (0.3, 1.0, 0.2), (0.03, -0.02, 0.04))
    src = ER.transform_points(v, np.linalg.inv(T_true))       # the target seen from a displaced frame
    T, fit, rmse, it = ER.icp(src, v, 0.1, max_iteration=60)
    assert fit == 1.0 and rmse < 1e-7 and 1 <= it <= 60
    np.testing.assert_allclose(T, T_true, rtol=0, atol=1e-6)


def test_restated_icp_keeps_a_sim3_initial_scale(room_mesh):
    v, _ = room_mesh
    s = 1.3
    T_true = rigid(2.0, (1.0, 0.2, -0.4), (0.02, 0.01, -0.03))
    S = np.diag([s, s, s, 1.0])
    src = ER.transform_points(v, np.linalg.inv(T_true @ S))     # scaled down and displaced
    init = S.copy()
    T, fit, rmse, _ = ER.icp(src, v, 0.1, trans_init=init, max_iteration=60)
    np.testing.assert_allclose(T, T_true @ S, rtol=0, atol=1e-6)
    assert abs(np.cbrt(np.linalg.det(T[:3, :3])) - s) < 1e-9 and fit == 1.0


def test_restated_icp_without_correspondences():
    T, fit, rmse, it = ER.icp(np.zeros((5, 3)), np.full((4, 3), 10.0), 0.1)
    assert np.array_equal(T, np.eye(4)) and fit == 0.0 and rmse == 0.0 and it == 1


def sphere_mesh(r, n=64):
    th = np.linspace(0, np.pi, n + 1)[1:-1]
    ph = np.linspace(0, 2 * np.pi, 2 * n, endpoint=False)
    v = [[0, 0, r]] + [[r * np.sin(t) * np.cos(p), r * np.sin(t) * np.sin(p), r * np.cos(t)] for t in th for p in ph] \
        + [[0, 0, -r]]
    m = 2 * n
    f = [[0, 1 + j, 1 + (j + 1) % m] for j in range(m)]
    for i in range(len(th) - 1):
        for j in range(m):
            a, b = 1 + i * m + j, 1 + i * m + (j + 1) % m
            f += [[a, a + m, b], [b, a + m, b + m]]
    last = 1 + (len(th) - 1) * m
    f += [[last + j, len(v) - 1, last + (j + 1) % m] for j in range(m)]
    return np.array(v), np.array(f)


@pytest.mark.parametrize("th,ratio", [(0.25, 100.0), (0.19, 0.0)])
def test_restated_metrics_of_concentric_spheres(th, ratio):
    """Radii 1 and 1 + delta: every nearest sample lies about delta away (plus the sample spacing, ~0.035 at 10^4
    samples, in quadrature), so accuracy ~ completion ~ delta and both ratios switch between 100 and 0 at dist_th."""
    delta = 0.2
    rng = np.random.RandomState(3)
    v1, f1 = sphere_mesh(1.0)
    v2, f2 = sphere_mesh(1.0 + delta)
    m = ER.eval_mesh(v2, f2, v1, f1, 10000, th, random=rng)
    assert abs(m["accuracy"] / 100 - delta) < 0.05 * delta and abs(m["completion"] / 100 - delta) < 0.05 * delta
    assert m["accuracy_ratio"] == ratio and m["completion_ratio"] == ratio


def test_sample_surface_matches_restatement_and_lies_on_faces():
    from go_slam_amd.neus.mesh import Mesh
    from go_slam_amd.neus.mesh_eval import sample_surface
    v, f = sphere_mesh(1.0, 16)
    np.random.seed(43)
    a = sample_surface(Mesh(v, f), 5000)
    np.random.seed(43)
    b = ER.sample_surface(v, f, 5000)
    assert np.array_equal(a, b)
    assert np.all(np.linalg.norm(a, axis=1) <= 1.0 + 1e-12) and np.all(np.linalg.norm(a, axis=1) > 0.98)


def test_metrics_file_layout(tmp_path, capsys):
    from go_slam_amd.neus import mesh_eval as ME
    m = ME.mesh_metrics(np.array([0.01, 0.02, 0.1]), np.array([0.03, 0.04]), 0.05)
    assert m == ER.metrics(np.array([0.01, 0.02, 0.1]), np.array([0.03, 0.04]), 0.05)
    txt = ME.metrics_text(m)
    lines = txt.split("\n")
    assert lines[:2] == ["", ""] and lines[2] == "Metrics of reconstructed mesh are:"
    assert lines[3:8] == ["\tAccuracy: 4.33cm", "\tCompletion: 3.50cm", "\tAccuracy Ratio: 66.67%",
                          "\tCompletion Ratio: 100.00%", "\tF-score: 80.00%"]
    assert txt.endswith("%\n\n")


def _write_ply(path, fmt, vdtype, extra, quads, colour):
    """A PLY written here field by field: 5 vertices (with normals / alpha when `extra`), 2 faces."""
    v = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0.5, 0.5, 1.25]], dtype=np.float64)
    c = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [9, 9, 9], [1, 2, 3]], dtype=np.uint8)
    faces = [[0, 1, 2, 3], [0, 1, 4]] if quads else [[0, 1, 2], [0, 1, 4]]
    t = {"f4": "float", "f8": "double"}[vdtype]
    head = ["ply", f"format {fmt} 1.0", "comment written by the test", "element vertex 5", f"property {t} x"]
    if extra:
        head += [f"property {t} nx"]
    head += [f"property {t} y", f"property {t} z"]
    if extra:
        head += ["property float ny", "property uchar alpha"]
    if colour:
        head += ["property uchar red", "property uchar green", "property uchar blue"]
    head += ["element face 2", "property list uchar uint vertex_index" if extra else "property list uchar int vertex_indices",
             "end_header"]
    with open(path, "wb") as fh:
        fh.write(("\n".join(head) + "\n").encode())
        e = "<" if fmt == "binary_little_endian" else ">"
        for i in range(5):
            vals = [(v[i, 0], vdtype)] + ([(0.5, vdtype)] if extra else []) + [(v[i, 1], vdtype), (v[i, 2], vdtype)]
            vals += [(0.25, "f4"), (7, "u1")] if extra else []
            vals += [(int(x), "u1") for x in c[i]] if colour else []
            if fmt == "ascii":
                fh.write((" ".join(repr(float(a)) if k.startswith("f") else str(a) for a, k in vals) + "\n").encode())
            else:
                fh.write(b"".join(np.array([a], dtype=e + k).tobytes() for a, k in vals))
        for fc in faces:
            if fmt == "ascii":
                fh.write((" ".join(str(x) for x in [len(fc)] + fc) + "\n").encode())
            else:
                fh.write(np.array([len(fc)], dtype="u1").tobytes() + np.array(fc, dtype=e + ("u4" if extra else "i4")).tobytes())
    return v, c


@pytest.mark.parametrize("fmt", ["ascii", "binary_little_endian", "binary_big_endian"])
@pytest.mark.parametrize("vdtype,extra,quads,colour", [("f4", False, False, False), ("f8", True, True, True),
                                                       ("f8", False, True, False), ("f4", True, False, True)])
def test_ply_reader(tmp_path, fmt, vdtype, extra, quads, colour):
    from go_slam_amd.neus.mesh import load_mesh
    v, c = _write_ply(str(tmp_path / "m.ply"), fmt, vdtype, extra, quads, colour)
    m = load_mesh(str(tmp_path / "m.ply"))
    assert m.vertices.dtype == np.float64 and np.array_equal(m.vertices, v.astype(vdtype).astype(np.float64))
    want = [[0, 1, 2], [0, 2, 3], [0, 1, 4]] if quads else [[0, 1, 2], [0, 1, 4]]
    assert np.array_equal(m.faces, want)
    assert (m.vertex_colors is None) == (not colour)
    if colour:
        assert np.array_equal(m.vertex_colors, c)


def test_ply_round_trip_through_export(tmp_path, room_mesh):
    from go_slam_amd.neus.mesh import Mesh, load_mesh
    v, f = room_mesh
    col = (np.arange(len(v) * 3) % 251).astype(np.uint8).reshape(-1, 3)
    for colours in (None, col):
        m = Mesh(v, f, colours)
        back = load_mesh(m.export(str(tmp_path / "r.ply")))
        assert np.array_equal(back.vertices, m.vertices) and np.array_equal(back.faces, m.faces)
        assert (back.vertex_colors is None and colours is None) or np.array_equal(back.vertex_colors, col)


def test_apply_transform_in_place_and_winding():
    from go_slam_amd.neus.mesh import Mesh
    v, f = sphere_mesh(1.0, 8)

    def signed_volume(m):
        t = m.vertices[m.faces]
        return np.einsum("ij,ij->i", t[:, 0], np.cross(t[:, 1], t[:, 2])).sum() / 6.0

    m = Mesh(v, f)
    vol = signed_volume(m)
    T = rigid(30, (1, 2, 3), (1, 2, 3))
    assert m.apply_transform(T) is m
    np.testing.assert_allclose(m.vertices, v @ T[:3, :3].T + T[:3, 3], rtol=0, atol=1e-14)
    assert np.array_equal(m.faces, f) and abs(signed_volume(m) - vol) < 1e-12
    mirror = np.diag([-1.0, 1.0, 1.0, 1.0])
    m.apply_transform(mirror)
    assert np.array_equal(m.faces, f[:, ::-1]) and abs(signed_volume(m) - vol) < 1e-12   # still outward
