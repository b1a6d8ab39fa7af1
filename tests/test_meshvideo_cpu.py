"""The mesh video without a GPU: go_slam_amd.meshvideo's scene state against what the reference's own module handed to
Open3D (tests/golden/meshvideo.npz, tests/golden/gen_golden_meshvideo.py), and the CPU restatements of the kernel
contracts (tests/meshvideo_restatement.py) on cases that can be checked by hand."""
import os
import sys

import numpy as np
import pytest

import meshvideo_restatement as MR

HERE = os.path.dirname(os.path.abspath(__file__))
TOL = 1e-12


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(HERE, "golden", "meshvideo.npz")))


def write_mesh(path, seed):
    from go_slam_amd.neus.mesh import Mesh
    g = np.random.default_rng(seed)
    Mesh(g.normal(size=(5, 3)), np.array([[0, 1, 2], [2, 3, 4]]), g.integers(0, 256, (5, 3)).astype(np.uint8)).export(path)
    return path


def drive(video, inp, with_reset, tmp_path):
    """the sequence of tests/golden/gen_golden_meshvideo.py::drive"""
    video.update_pose(3, inp["pose_a"].copy())
    video.update_pose(5, inp["pose_kf"].copy(), is_keyframe=True)
    video.update_pose(3, inp["pose_gt"].copy(), is_gt=True)
    video.update_mesh(write_mesh(str(tmp_path / "mesh_a.ply"), 1))
    video.update_pose(3, inp["pose_a2"].copy())
    video.update_cam_trajectory(int(inp["traj_i_est"]), False)
    video.update_cam_trajectory(int(inp["traj_i_gt"]), True)
    video.update_mesh(write_mesh(str(tmp_path / "mesh_b.ply"), 2))
    video.update_cam_trajectory(int(inp["traj_i_est"]) - 2, False)
    if with_reset:
        video.reset()
        video.update_pose(8, inp["pose_after"].copy())


def same_set(g, tag, points, lines, colors):
    assert np.abs(points - g[tag + "_points"]).max() <= TOL
    assert lines.dtype.kind == "i" and np.array_equal(lines, g[tag + "_lines"])
    assert np.abs(colors - g[tag + "_colors"]).max() <= TOL


@pytest.mark.parametrize("is_gt", [False, True])
@pytest.mark.parametrize("is_keyframe", [False, True])
def test_camera_actor_matches_reference(golden, is_gt, is_keyframe):
    from go_slam_amd.meshvideo import camera_actor
    pts, lines, cols = camera_actor(is_gt, is_keyframe, float(golden["cam_scale"]))
    same_set(golden, f"actor_gt{int(is_gt)}_kf{int(is_keyframe)}", pts, lines, cols)
    assert pts.shape == (8, 3) and lines.shape == (12, 2)


@pytest.mark.parametrize("with_reset", [False, True])
def test_scene_state_matches_reference(golden, with_reset, tmp_path):
    from go_slam_amd.meshvideo import GT_ID_OFFSET, MeshVideo
    g, tag = golden, "reset" if with_reset else "run"
    video = MeshVideo(str(tmp_path), g["init_pose"].copy(), cam_scale=float(g["cam_scale"]),
                      estimate_c2w_list=g["est_c2w"], gt_c2w_list=g["gt_c2w"], render=False).start()
    drive(video, g, with_reset, tmp_path)
    assert np.abs(video.extrinsic - g[f"{tag}_extrinsic"]).max() <= TOL
    # the reference's visualiser holds its line sets in insertion order: cameras, the ground-truth trajectory, the
    # estimated one (replaced last); after the reset the cameras are gone and the new one comes last
    cams = [0, 1, 2] if not with_reset else [2]
    traj_gt, traj_est = (3, 4) if not with_reset else (0, 1)
    assert int(g[f"{tag}_n_sets"]) == len(video.cameras) + 2
    assert list(video.cameras) == ([3, 5, 3 + GT_ID_OFFSET] if not with_reset else [8])
    for j, actor in zip(cams, video.cameras.values()):
        same_set(g, f"{tag}_set{j}", actor[0], actor[1], actor[2])
        assert np.abs(actor[4] - g[f"{tag}_set{j}_transforms"][-1]).max() <= TOL
    same_set(g, f"{tag}_set{traj_gt}", *video.traj_actor_gt)
    same_set(g, f"{tag}_set{traj_est}", *video.traj_actor)
    # the mesh is the second file, with its colours
    ref = np.random.default_rng(2)
    assert np.allclose(video.mesh.vertices, ref.normal(size=(5, 3))) and video.mesh.vertex_colors.shape == (5, 3)
    segs, cols = video.scene()
    assert segs.shape == (sum(len(g[f"{tag}_set{j}_lines"]) for j in range(int(g[f"{tag}_n_sets"]))), 2, 3)
    assert cols.shape == (len(segs), 3)


def test_update_pose_edits_the_pose_in_place(golden, tmp_path):
    from go_slam_amd.meshvideo import MeshVideo
    video = MeshVideo(str(tmp_path), golden["init_pose"].copy(), render=False)
    p = golden["pose_a"].copy()
    video.update_pose(11, p, is_gt=True, is_keyframe=True)
    assert np.array_equal(p, golden["enqueued_pose"]) and video.cameras[11 + int(1e8)][3] is p
    assert video.start() is video and video.frame() is None


def test_defaults_and_dropin():
    from go_slam_amd import dropin, meshvideo
    fx, fy, cx, cy = meshvideo.default_intrinsics(1080, 1920)
    assert fx == fy and abs(fy - 540.0 / np.tan(np.pi / 6)) < 1e-9 and (cx, cy) == (959.5, 539.5)
    saved = {k: sys.modules.get(k) for k in ("src.tools.meshvideo", "droid_backends", "tinycudann", "lietorch",
                                             "torch_scatter")}
    try:
        sys.modules.pop("src.tools.meshvideo", None)
        dropin.install(droid_backends=False, tinycudann=False, lietorch=False, torch_scatter=False)
        assert "src.tools.meshvideo" not in sys.modules
        dropin.install(droid_backends=False, tinycudann=False, lietorch=False, torch_scatter=False, meshvideo=True)
        assert sys.modules["src.tools.meshvideo"].MeshVideo is meshvideo.MeshVideo
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


# ---- the restatements on cases checked by hand --------------------------------------------------------------------
EYE = np.eye(4)[:3]
CAM = dict(H=12, W=16, fx=10.0, fy=10.0, cx=8.0, cy=6.0)


def test_restated_axis_aligned_segment():
    """From (-0.3, 0.05, 1) to (0.4, 0.05, 1): u from 5 to 12, v = 6.5: columns 5..12 of row 6, all at depth 1."""
    st = MR.line_steps([[-0.3, 0.05, 1.0], [0.4, 0.05, 1.0]], EYE, **CAM)
    assert st[:, 0].tolist() == [6.0] * 8 and st[:, 1].tolist() == list(range(5, 13))
    assert np.allclose(st[:, 2], 1.0)
    # a point: one step
    st = MR.line_steps([[0.0, 0.0, 2.0], [0.0, 0.0, 2.0]], EYE, **CAM)
    assert st[:, :3].tolist() == [[6.0, 8.0, 2.0]]


def test_restated_segment_across_the_near_plane():
    """From (0.05, 0.05, -1) behind the camera to (0.05, 0.05, 1): clipped at z = 0.5, not dropped.  The clipped end is
    (0.05, 0.05, 0.5) -> (u, v) = (9, 7); the far end (8.5, 6.5): the steps are pixels (7, 9) and (6, 8), at depths 0.5
    and 1 -- 1/z is linear along the projected line."""
    st = MR.line_steps([[0.05, 0.05, -1.0], [0.05, 0.05, 1.0]], EYE, znear=0.5, **CAM)
    assert st[:, :2].tolist() == [[7.0, 9.0], [6.0, 8.0]] and np.allclose(st[:, 2], [0.5, 1.0])
    assert len(MR.line_steps([[0.05, 0.05, -1.0], [0.05, 0.05, 0.4]], EYE, znear=0.5, **CAM)) == 0
    # hidden by a nearer surface, in front of a farther one
    tri = np.array([[-5.0, -5.0, 0.75], [5.0, -5.0, 0.75], [0.0, 5.0, 0.75]])
    buf = MR.Buffer(1, CAM["H"], CAM["W"])
    MR.mesh_visbuf(buf, tri, [[0, 1, 2]], EYE[None], znear=0.5, **CAM)
    MR.line_visbuf(buf, [[[0.05, 0.05, -1.0], [0.05, 0.05, 1.0]]], 1, EYE[None], znear=0.5, **CAM)
    assert buf.id[0, 7, 9] == 1 and buf.id[0, 6, 8] == 0 and (buf.id >= 0).all()


def test_restated_tetrahedron_normals():
    """The corner tetrahedron (0, e1, e2, e3), faces wound outward.  At the origin the three coordinate faces add
    (-1, -1, -1); at e1 the faces z = 0, y = 0 and the slanted one (cross product (1, 1, 1)) add (1, 0, 0).  With
    scale 2^20 every cross product is an integer multiple of the quantum, so the sums are exact."""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [5, 5, 5]], np.float64)
    f = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3], [1, 1, 2]])
    scale = 2.0 ** 20
    sums, exact, valence = MR.normal_sums(v, f, scale)
    assert [int(x) for x in sums[0]] == [-(1 << 20)] * 3 and [int(x) for x in sums[1]] == [1 << 20, 0, 0]
    assert valence.tolist() == [3, 5, 4, 3, 0]                 # the zero-area face counts, and adds nothing
    n = MR.vertex_normals(v, f, scale)
    assert np.allclose(n[0], -np.ones(3) / np.sqrt(3), atol=1e-7) and n[1].tolist() == [1.0, 0.0, 0.0]
    assert n[4].tolist() == [0.0, 0.0, 0.0]                    # unreferenced
    assert np.array_equal(MR.vertex_normals(v, f[[4]], scale), np.zeros((5, 3), np.float32))


def test_restated_resolve_of_one_face():
    """A triangle in the plane z = 2 seen head-on, vertex colours red / green / blue, flat: at the pixel whose ray meets
    the centroid the albedo is 85 per channel and the cosine that of the ray to the axis."""
    tri = np.array([[-1.0, -1.0, 2.0], [1.0, -1.0, 2.0], [0.0, 2.0, 2.0]])
    cam = dict(fx=10.0, fy=10.0, cx=7.5, cy=5.5)               # pixel (5, 7) looks down the axis: the centroid (0, 0, 2)
    ids = np.full((1, 12, 16), -1, np.int64)
    ids[0, 5, 7], ids[0, 0, 0] = 0, 1
    cols = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255]])
    img = MR.resolve(ids, tri, [[0, 1, 2]], EYE[None], vertex_colors=cols, flat=True, line_colors=np.array([[9, 8, 7]]),
                     **cam)
    assert img[0, 5, 7].tolist() == [85, 85, 85]               # 85 * (0.3 + 0.7 * 1)
    assert img[0, 0, 0].tolist() == [9, 8, 7] and img[0, 3, 3].tolist() == [255, 255, 255]
    n = np.tile(np.array([[0.0, 0.6, 0.8]]), (3, 1))            # smooth normals tilted by acos(0.8)
    img = MR.resolve(ids, tri, [[0, 1, 2]], EYE[None], normals=n, line_colors=np.array([[9, 8, 7]]), **cam)
    assert img[0, 5, 7].tolist() == [int(np.rint(178.5 * (np.float32(0.3) + np.float32(0.7) * 0.8)))] * 3
