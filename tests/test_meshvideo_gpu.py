"""The mesh video on the MI355X against the CPU restatements (tests/meshvideo_restatement.py): the visibility buffer
against gs_mesh_depth and the restated nearest face, the shaded image, the fixed-point vertex normals, the depth-tested
lines, bitwise reruns, and MeshVideo end to end.  Scenes and poses are those of test_mesher_gpu.py."""
import json
import os

import numpy as np
import pytest
import torch

import cull_restatement as CR
import meshvideo_restatement as MR
from test_mesher_cpu import sphere
from test_mesher_gpu import blob_mesh, look_at

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAR = 20.0
SPHERE_C, EYE0 = np.array([0.3, 0.2, 0.1]), np.array([3.0, 0.5, 0.7])


def scene():
    """sphere plus blob, vertex colours, the four poses (the last two inside the mesh)"""
    sv, sf = sphere(10, 1.0)
    bv, bf = blob_mesh(1, 16)
    v = np.concatenate([sv * 0.4 + SPHERE_C, bv]).astype(np.float32)
    f = np.concatenate([sf, bf + len(sv)])
    col = np.random.default_rng(3).integers(0, 256, (len(v), 3)).astype(np.uint8)
    poses = np.stack([look_at(EYE0, (0, 0, 0)), look_at((-0.2, 2.6, -1.1), (0.1, 0, 0)),
                      look_at((0.05, 0.1, 0.02), (1, 0.3, 0.2)), look_at((0.3, -0.2, 0.1), (-1, -0.2, 0.4))])
    return v, f, col, poses.astype(np.float32)


def camera(H, W):
    return dict(fx=0.8 * W, fy=0.8 * W, cx=W / 2 - 0.3, cy=H / 2 + 0.2)


def split(vb):
    """(depth bits uint32, id int64 with -1 for empty) of a visibility buffer"""
    vb = vb.cpu().numpy()
    ids = (vb & 0xffffffff).astype(np.int64)
    ids[vb == -1] = -1
    return ((vb >> 32) & 0xffffffff).astype(np.uint32), ids


def record(key, value):
    """keep a measured figure beside the benchmark's (profiles/meshvideo.json); a read-only tree just skips it"""
    path = os.path.join(ROOT, "profiles", "meshvideo.json")
    try:
        data = json.load(open(path)) if os.path.exists(path) else {}
        data.setdefault("tests", {})[key] = value
        json.dump(data, open(path, "w"), indent=1)
    except OSError:
        pass


@pytest.mark.parametrize("H,W", [(48, 64), (240, 320)])
def test_visbuf_ids_and_colour_match_restatement(built_lib, H, W):
    """High word = gs_mesh_depth's map bit for bit; face = the restatement's nearest face at every pixel that is not
    ambiguous (flagged by cull_restatement.mesh_depth, or two nearest fragments within 1e-6 relative; below 5 % of the
    pixels); colour within one level of the restatement there: both evaluate the same fp64 expression and round once, so
    they differ only where albedo * shade sits within their rounding noise of a half-integer."""
    from go_slam_amd import meshvideo as MV
    from go_slam_amd.neus.mesher import render_mesh_depth
    v, f, col, poses = scene()
    cam = camera(H, W)
    mesh = MV.upload_mesh((v, f, col), DEV)
    w2c = MV.world_to_camera(torch.from_numpy(poses), DEV)
    vb = MV.render_visbuf(mesh, w2c, H, W, **cam, far=FAR)
    bits, ids = split(vb)
    depth = render_mesh_depth((v, f), torch.from_numpy(poses), H, W, cam["fx"], cam["fy"], cam["cx"], cam["cy"],
                              far=FAR).cpu().numpy()
    hit = depth > 0
    assert np.array_equal(bits[hit], depth.view(np.uint32)[hit])
    assert (vb.cpu().numpy()[~hit] == -1).all() and (ids[hit] >= 0).all()

    M = w2c.cpu().numpy().astype(np.float64)
    buf = MR.Buffer(len(M), H, W)
    MR.mesh_visbuf(buf, v, f, M, H, W, **cam, far=FAR)
    _, amb = CR.mesh_depth(v.astype(np.float64), f, poses.astype(np.float64), H, W, cam["fx"], cam["fy"], cam["cx"],
                           cam["cy"], far=FAR)
    amb = amb | buf.close_pairs()
    print("ambiguous share", amb.mean(), "covered", hit.mean())
    assert amb.mean() < 0.05 and hit.mean() > 0.2
    ok = ~amb
    assert np.array_equal(ids[ok], buf.id[ok]), int((ids != buf.id)[ok].sum())

    normals, _, scale = MV.vertex_normals(v, f, DEV, return_sums=True)
    ref_n = MR.vertex_normals(v, f, scale)
    for flat in (False, True):
        got = MV.resolve_visbuf(vb, mesh, w2c, **cam, flat=flat).cpu().numpy()
        ref = MR.resolve(buf.id, v, f, M, **cam, vertex_colors=col, normals=ref_n, flat=flat)
        diff = np.abs(got.astype(np.int16) - ref.astype(np.int16)).max(-1)
        share = float((diff[ok] == 0).mean())
        print("flat", flat, "max level difference", diff[ok].max(), "exactly equal share", share)
        record(f"colour_exact_share_{H}x{W}_{'flat' if flat else 'smooth'}", share)
        assert diff[ok].max() <= 1
    grey = MV.resolve_visbuf(vb, MV.DeviceMesh(mesh.vertices, mesh.faces, None, mesh.normals), w2c, **cam).cpu().numpy()
    assert (grey[~hit] == 255).all() and (grey[hit].max(-1) <= 179).all() and (np.ptp(grey[hit], axis=-1) == 0).all()


def test_vertex_normals_fixed_point_bound(built_lib):
    """Two runs are bit-identical, and each is within the fixed-point bound.  With q = 1 / scale the quantum: a face's
    cross-product component x becomes rint(x * scale) -- the product is exact, scale being a power of two -- so it is off
    by at most q / 2; integer sums are exact; a vertex of valence m therefore has |S / scale - sum x| <= m q / 2 per
    component (plus the float64 reference's own rounding, below m 2^-52 max |x|).  For the unit normal: with N the exact
    sum and d the error vector, |N + d| / |N + d| - N / |N|| <= 2 |d| / |N|, |d| <= sqrt(3) m q / 2, plus 2^-24 for the
    one rounding to float32 (the sums' conversion to float64 adds 2^-53 relative, covered by 1e-15)."""
    from go_slam_amd import meshvideo as MV
    v, f, _, _ = scene()
    f = np.concatenate([f, [[0, 0, 1], [2, 2, 2]]])                  # zero-area faces
    v = np.concatenate([v, [[9.0, 9.0, 9.0]]]).astype(np.float32)     # an unreferenced vertex
    n1, s1, scale = MV.vertex_normals(v, f, DEV, return_sums=True)
    n2, s2, _ = MV.vertex_normals(v, f, DEV, return_sums=True)
    assert torch.equal(s1, s2) and torch.equal(n1.view(torch.int32), n2.view(torch.int32))
    assert scale == MV.normal_scale(torch.from_numpy(v), len(f)) and np.log2(scale) == int(np.log2(scale))
    _, exact, valence = MR.normal_sums(v, f, scale)
    q = 1.0 / scale
    sums = s1.cpu().numpy().astype(np.float64) * q
    cross_max = 12.0 * float(np.abs(v).max()) ** 2                    # |a x b| <= |a| |b|, |a|, |b| <= 2 sqrt(3) max |v|
    bound = valence[:, None] * (0.5 * q + 2.0 ** -52 * cross_max) + 1e-15 * np.abs(exact)
    print("scale 2^%d" % int(np.log2(scale)), "max valence", valence.max(), "worst sum error / bound",
          (np.abs(sums - exact) / np.maximum(bound, 1e-300)).max())
    assert (np.abs(sums - exact) <= bound).all()
    length = np.linalg.norm(exact, axis=1)
    has = length > 0
    unit = exact[has] / length[has, None]
    nbound = 2.0 * np.sqrt(3.0) * np.linalg.norm(bound[has], axis=1) / length[has] + 2.0 ** -24 + 1e-15
    err = np.linalg.norm(n1.cpu().numpy().astype(np.float64)[has] - unit, axis=1)
    print("worst normal error / bound", (err / nbound).max())
    assert (err <= nbound).all()
    assert not n1[-1].any() and has[:-1].mean() > 0.99


def line_scene():
    g = np.random.default_rng(11)
    segs = list(g.uniform(-1.2, 1.2, (24, 2, 3)))
    fwd = (SPHERE_C - EYE0) / np.linalg.norm(SPHERE_C - EYE0)
    side = np.cross(fwd, [0.0, 0.0, 1.0])
    side /= np.linalg.norm(side)
    front = EYE0 + 0.5 * (SPHERE_C - EYE0)          # outside the blob's box: nothing between it and the first camera
    behind = SPHERE_C + 0.6 * fwd                    # in the sphere's shadow
    segs += [np.stack([front - 0.1 * side, front + 0.1 * side]), np.stack([behind - 0.15 * side, behind + 0.15 * side])]
    segs = np.asarray(segs, np.float32)
    return segs, g.integers(0, 256, (len(segs), 3)).astype(np.uint8)


@pytest.mark.parametrize("H,W", [(48, 64), (240, 320)])
def test_lines_own_the_restated_pixels(built_lib, H, W):
    """The pixels owned by line ids are the restatement's, away from steps within 1e-3 px of a rounding boundary, from
    pixels the surface's own coverage leaves open, and from fragments within 1e-6 relative of each other."""
    from go_slam_amd import meshvideo as MV
    v, f, col, poses = scene()
    segs, scol = line_scene()
    cam = camera(H, W)
    mesh = MV.upload_mesh((v, f, col), DEV)
    w2c = MV.world_to_camera(torch.from_numpy(poses), DEV)
    vb = MV.render_visbuf(mesh, w2c, H, W, **cam, segments=torch.from_numpy(segs).to(DEV), far=FAR)
    _, ids = split(vb)
    M = w2c.cpu().numpy().astype(np.float64)
    buf = MR.Buffer(len(M), H, W)
    MR.mesh_visbuf(buf, v, f, M, H, W, **cam, far=FAR)
    unsure = MR.line_visbuf(buf, segs, len(f), M, H, W, **cam, far=FAR)
    _, amb = CR.mesh_depth(v.astype(np.float64), f, poses.astype(np.float64), H, W, cam["fx"], cam["fy"], cam["cx"],
                           cam["cy"], far=FAR)
    ok = ~(unsure | amb | buf.close_pairs())
    print("excluded share", 1 - ok.mean(), "line pixels", (buf.id >= len(f)).sum())
    assert ok.mean() > 0.9 and (buf.id >= len(f))[ok].sum() > 50
    assert np.array_equal(ids[ok], buf.id[ok]), int((ids != buf.id)[ok].sum())
    # in front of everything: every step owned; in the sphere's shadow: none
    front, behind = len(f) + len(segs) - 2, len(f) + len(segs) - 1
    for sid, owned in ((front, True), (behind, False)):
        st = MR.line_steps(segs[sid - len(f)], M[0], H, W, **cam, far=FAR)
        st = st[st[:, 3] >= 1e-3]
        assert len(st) >= 2
        r, c = st[:, 0].astype(int), st[:, 1].astype(int)
        assert ((ids[0, r, c] == sid) == owned).all() and ((ids[0] == sid).sum() > 0) == owned
    img = MV.resolve_visbuf(vb, mesh, w2c, **cam, line_colors=torch.from_numpy(scol).to(DEV)).cpu().numpy()
    line = ids >= len(f)
    assert np.array_equal(img[line], scol[ids[line] - len(f)])


def test_segment_across_the_near_plane_is_clipped(built_lib):
    from go_slam_amd import meshvideo as MV
    H, W = 48, 64
    cam = dict(fx=50.0, fy=50.0, cx=32.0, cy=24.0)
    seg = np.array([[[0.3, 0.2, -1.0], [-0.2, -0.1, 2.0]], [[0.1, 0.1, -3.0], [0.2, 0.1, -1.0]]], np.float32)
    w2c = MV.world_to_camera(torch.eye(4)[None], DEV)
    vb = MV.render_visbuf(MV.upload_mesh(None, DEV), w2c, H, W, **cam, segments=torch.from_numpy(seg).to(DEV), near=0.5)
    _, ids = split(vb)
    buf = MR.Buffer(1, H, W)
    unsure = MR.line_visbuf(buf, seg, 0, np.eye(4)[None, :3], H, W, **cam, znear=0.5)
    assert (buf.id == 0).sum() > 10 and not (buf.id == 1).any()          # the second one is wholly behind the plane
    assert np.array_equal(ids[~unsure], buf.id[~unsure])
    bits = split(vb)[0]
    assert bits[ids == 0].view(np.float32).min() >= 0.5


def test_reruns_are_bitwise_identical(built_lib):
    from go_slam_amd import meshvideo as MV
    v, f, col, poses = scene()
    segs, scol = line_scene()
    cam = camera(120, 160)
    out = [MV.render_mesh_frames((v, f, col), torch.from_numpy(poses), 120, 160, **cam, lines=segs, line_colors=scol,
                                 far=FAR, chunk=3) for _ in range(2)]
    assert torch.equal(out[0], out[1]) and out[0].shape == (4, 120, 160, 3) and out[0].dtype == torch.uint8
    mesh = MV.upload_mesh((v, f, col), DEV)
    w2c = MV.world_to_camera(torch.from_numpy(poses), DEV)
    vbs = [MV.render_visbuf(mesh, w2c, 120, 160, **cam, segments=torch.from_numpy(segs).to(DEV), far=FAR)
           for _ in range(2)]
    assert torch.equal(vbs[0], vbs[1])
    one = MV.render_mesh_frames(mesh, torch.from_numpy(poses[1:2]), 120, 160, **cam, lines=segs, line_colors=scol, far=FAR)
    assert torch.equal(one[0], out[0][1])


def test_meshvideo_end_to_end(built_lib, tmp_path):
    from PIL import Image
    from go_slam_amd import meshvideo as MV
    from go_slam_amd.neus.mesh import Mesh, load_mesh
    v, f, col, _ = scene()
    path = Mesh(v, f, col).export(str(tmp_path / "00050_mesh.ply"))
    g = np.random.default_rng(5)
    est = np.stack([look_at(g.normal(size=3) * 0.3 + [2.0, 0.0, 0.0], (0, 0, 0)) for _ in range(8)])
    gt = est.copy()
    gt[:, :3, 3] += 0.05
    H, W = 120, 160
    # the first frame's pose for which the viewer ends up at (3, 0.4, 0.5) looking at the origin (viewer_extrinsic)
    view = look_at((3.0, 0.4, 0.5), (0, 0, 0))
    init = view.copy()
    init[:3, 1:3] *= -1
    init[:3, 3] = view[:3, 3] - 2 * init[:3, 2]
    video = MV.MeshVideo(str(tmp_path), init, cam_scale=0.2, save_rendering=True, estimate_c2w_list=torch.from_numpy(est),
                         gt_c2w_list=gt, height=H, width=W, device=DEV).start()
    assert np.allclose(video.view_c2w, view, atol=1e-12)
    video.update_mesh(path)
    video.update_pose(1, est[1].copy())
    video.update_pose(1, gt[1].copy(), is_gt=True)
    video.update_cam_trajectory(8, False)
    video.update_cam_trajectory(8, True)
    video.join()
    names = sorted(os.listdir(tmp_path / "tmp_rendering"))
    assert names == [f"{i:06d}.jpg" for i in range(1, 6)]
    for n in names:
        assert Image.open(tmp_path / "tmp_rendering" / n).size == (W, H)
    segs, cols = video.scene()
    assert segs.shape == (12 + 12 + 6 + 6, 2, 3)
    fx, fy, cx, cy = video.intrinsics
    direct = MV.render_mesh_frames(load_mesh(path), video.view_c2w[None], H, W, fx, fy, cx, cy, lines=segs,
                                   line_colors=cols, near=video.near, device=DEV)[0]
    frame = video.frame()
    assert frame.is_cuda and torch.equal(frame, direct)
    px = frame.cpu().numpy().reshape(-1, 3)
    assert (px == [0, 0, 255]).all(1).any() and (px == [0, 255, 0]).all(1).any()      # both kinds of line survive
    assert 0.05 < (px != 255).any(1).mean() < 1.0                                       # and the mesh is in view
