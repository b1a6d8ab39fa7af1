"""tests/tsdf_restatement.py against truth that does not come from it -- a fronto-parallel plane whose TSDF and
observation counts are known in closed form, hand-built boundary cases -- and the argument checks of go_slam_amd.tsdf
that need no GPU."""
import os
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import tsdf_restatement as TR                                  # noqa: E402

C = 2.013
U32 = 2.0 ** -23


def fuse_plane(c, dtype):
    dims = TR.lattice_dims(TR.PLANE_BOUND, TR.PLANE_VOXEL)
    depth, w2c = TR.plane_scene(c)
    if dtype is np.float64:          # the analytic run takes the scene's exact numbers, not their fp32 roundings
        depth = np.stack([np.full(TR.PLANE_HW, c - q[2]) for q in TR.PLANE_CAMS])
        w2c = w2c.astype(np.float64)
        w2c[:, :, 3] = -TR.PLANE_CAMS
    vol = TR.integrate(TR.new_volume(dims, dtype), depth, w2c, TR.PLANE_INTR, TR.PLANE_BOUND[:, 0], TR.PLANE_VOXEL,
                       4 * TR.PLANE_VOXEL, dtype=dtype)
    return dims, vol


def test_plane_tsdf_is_the_closed_form():
    trunc = 4 * TR.PLANE_VOXEL
    dims, vol = fuse_plane(C, np.float64)
    z = (TR.PLANE_BOUND[2, 0] + np.arange(dims[2]) * TR.PLANE_VOXEL)[None, None, :] * np.ones(dims)
    seen = vol["weight"] > 0
    assert seen.sum() > 0.2 * seen.size
    assert not seen[C - z < -trunc].any()                   # nothing is integrated farther than trunc behind the plane
    want = np.minimum(1.0, (C - z) / trunc)
    err = np.abs(vol["tsdf"] - want)[seen]
    print("fp64 max |tsdf - closed form| / |closed form|:", (err / np.abs(want[seen])).max())
    assert (err <= 2 * U32 * np.abs(want[seen])).all()      # 2 fp32 ulps of the value
    # the fp32 restatement: d, pz and pc.z are each rounded at magnitudes below 4 (half an ulp: 2^-23 * 2 each), the
    # difference is exact or rounded once more, so |sdf error| <= 4 * 2^-22; over trunc, plus four roundings of the
    # running mean at magnitudes <= 1
    dims, vol32 = fuse_plane(C, np.float32)
    bound = 4 * 2.0 ** -22 / trunc + 4 * U32
    seen32 = vol32["weight"] > 0
    err32 = np.abs(vol32["tsdf"].astype(np.float64) - want)[seen32]
    print("fp32 max |tsdf - closed form|:", err32.max(), "bound", bound)
    assert err32.max() <= bound
    assert (vol32["tsdf"][~seen32] == 1).all() and (vol32["colors"] == 0).all()


def test_plane_weight_is_the_number_of_cameras_that_see_the_point():
    trunc = 4 * TR.PLANE_VOXEL
    dims, vol = fuse_plane(C, np.float32)
    count, shaky = TR.plane_projection_counts(dims)
    assert shaky.mean() < 0.01, shaky.mean()
    z = (TR.PLANE_BOUND[2, 0] + np.arange(dims[2]) * TR.PLANE_VOXEL)[None, None, :] * np.ones(dims)
    front = C - z >= -trunc
    assert abs(C - z + trunc).min() > 1e-4                  # no lattice plane sits on the truncation boundary
    sel = front & ~shaky
    assert set(np.unique(count[sel])) == {0, 1, 2, 3}
    assert np.array_equal(vol["weight"][sel], count[sel].astype(np.float32))
    assert (vol["weight"][~front] == 0).all()


def _one_camera(depth_value, **kw):
    """A 2 x 2 x 2 lattice at x, y = +-0.125, z = 1 and 1.25 in front of an identity camera; trunc = 0.25."""
    vol = TR.new_volume((2, 2, 2))
    depth = np.full((1, 8, 8), depth_value, np.float32)
    w2c = np.zeros((1, 3, 4), np.float32)
    w2c[0, :, :3] = np.eye(3)
    return TR.integrate(vol, depth, w2c, (8.0, 8.0, 3.5, 3.5), (-0.125, -0.125, 1.0), 0.25, 0.25, **kw)


def test_truncation_boundary():
    at = _one_camera(1.0)                                   # z = 1.25: sdf == -trunc exactly, integrated with s = -1
    assert (at["tsdf"][:, :, 1] == -1).all() and (at["weight"][:, :, 1] == 1).all()
    assert (at["tsdf"][:, :, 0] == 0).all() and (at["weight"][:, :, 0] == 1).all()
    below = _one_camera(np.nextafter(np.float32(1.0), np.float32(0.0)))      # sdf one ulp under -trunc: skipped
    assert np.float32(np.nextafter(np.float32(1.0), np.float32(0.0))) - np.float32(1.25) < np.float32(-0.25)
    assert (below["tsdf"][:, :, 1] == 1).all() and (below["weight"][:, :, 1] == 0).all()
    assert (below["weight"][:, :, 0] == 1).all()


def test_max_weight_caps_the_weight():
    vol = TR.new_volume((2, 2, 2))
    w2c = np.zeros((6, 3, 4), np.float32)
    w2c[:, :, :3] = np.eye(3)
    depth = np.stack([np.full((8, 8), 1.0 + 0.01 * f, np.float32) for f in range(6)])
    states = []
    for f in range(6):
        TR.integrate(vol, depth[f:f + 1], w2c[f:f + 1], (8.0, 8.0, 3.5, 3.5), (-0.125, -0.125, 1.0), 0.25, 0.25,
                     max_weight=4.0)
        states.append(float(vol["weight"][0, 0, 0]))
    assert states == [1.0, 2.0, 3.0, 4.0, 4.0, 4.0]
    # z = 1 plane: s_f = 0.04 f; running mean of f = 0..3, then two steps of (4 t + s) / 5
    t = np.mean([0.0, 0.04, 0.08, 0.12])
    t = (4 * t + 0.16) / 5
    t = (4 * t + 0.20) / 5
    assert abs(float(vol["tsdf"][0, 0, 0]) - t) < 1e-6


def test_masked_and_zero_depth_pixels_leave_their_points_untouched():
    fx, fy, cx, cy = 8.0, 8.0, 3.5, 3.5
    depth = np.full((1, 8, 8), 1.1, np.float32)
    mask = np.ones((1, 8, 8), np.float32)
    w2c = np.zeros((1, 3, 4), np.float32)
    w2c[0, :, :3] = np.eye(3)
    # the lattice points (x, y) = (-0.125, -0.125) and (0.125, 0.125) at z = 1 land on pixels (2.5 -> 3, 2.5 -> 3) and
    # (4.5 -> 5, 4.5 -> 5); at z = 1.25 on (2.7 -> 3, 2.7 -> 3) and (4.3 -> 4, 4.3 -> 4)
    mask[0, 3, 3] = 0.0
    depth[0, 5, 5] = 0.0
    vol = TR.integrate(TR.new_volume((2, 2, 2)), depth, w2c, (fx, fy, cx, cy), (-0.125, -0.125, 1.0), 0.25, 0.25,
                       mask=mask)
    assert (vol["tsdf"][0, 0] == 1).all() and (vol["weight"][0, 0] == 0).all()          # both z behind the masked pixel
    assert vol["tsdf"][1, 1, 0] == 1 and vol["weight"][1, 1, 0] == 0                     # the zero-depth pixel
    assert vol["weight"][1, 1, 1] == 1 and vol["weight"][0, 1, 0] == 1 and vol["weight"][1, 0, 1] == 1


def test_vertex_attr_blends_along_the_edge():
    weight = np.zeros((3, 3, 3), np.float32)
    weight[:2] = 2.0
    colors = np.zeros((3, 3, 3, 3), np.float32)
    colors[0, 1] = 1.0
    colors[1, :, 2] = 0.5
    verts = np.array([[0.25, 1, 1], [1, 1, 1], [1.5, 0, 0], [1, 1.75, 2], [0, 0, 0.5]], np.float32)
    keep, rgb = TR.vertex_attr(verts, weight, colors, 1.0)
    assert keep.tolist() == [True, True, False, True, True]
    assert rgb[0].tolist() == [0.25, 0.0, 0.0] and rgb[1].tolist() == [1.0, 0.0, 0.0]
    assert rgb[3].tolist() == [1.0, 0.375, 0.0] and rgb[4].tolist() == [0.0, 0.0, 0.0]


def test_too_many_lattice_points_names_the_axis():
    from go_slam_amd.tsdf import TSDFVolume
    with pytest.raises(ValueError, match="axis y"):
        TSDFVolume([[0, 1], [0, 10.3], [0, 1]], 0.01, device="cpu")
    with pytest.raises(ValueError, match="axis z"):
        TSDFVolume([[0, 1], [0, 1], [-60, 60]], 0.1, device="cpu")


def _stub_video(mode):
    return types.SimpleNamespace(disps_up=torch.zeros(4, 8, 8), cfg={"mode": mode}, counter=types.SimpleNamespace(value=2),
                                 filtered_id=torch.tensor([2]))


@pytest.mark.parametrize("mode", ["mono", "stereo"])
def test_sensor_source_needs_sensor_depth(mode):
    from go_slam_amd.tsdf import fuse_keyframes
    with pytest.raises(ValueError, match="sensor"):
        fuse_keyframes(_stub_video(mode), [[0, 1], [0, 1], [0, 1]], 0.1, source="sensor")


def test_filtered_source_takes_no_index():
    from go_slam_amd.tsdf import fuse_keyframes
    with pytest.raises(ValueError, match="index must be None"):
        fuse_keyframes(_stub_video("rgbd"), [[0, 1], [0, 1], [0, 1]], 0.1, source="filtered", index=[0])
    with pytest.raises(ValueError, match="unknown source"):
        fuse_keyframes(_stub_video("rgbd"), [[0, 1], [0, 1], [0, 1]], 0.1, source="depth")


def test_absent_or_disabled_key_does_nothing():
    from go_slam_amd.tsdf import fuse_from_config
    for cfg in ({}, {"tsdf": None}, {"tsdf": {"enable": False, "source": "sensor"}}):
        assert fuse_from_config(types.SimpleNamespace(cfg=cfg)) is None
