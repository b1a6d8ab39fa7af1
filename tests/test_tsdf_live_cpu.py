"""tests/tsdf_live_restatement.py against truth that does not come from it -- the fronto-parallel plane of
tsdf_restatement whose counts are known in closed form, the fp64 mean of the unquantised observations, hand-built
boundary cases -- its linearity, `plan_refresh`, the refusals of go_slam_amd.tsdf_live that need no GPU, and the compiled
kernels' register and scratch budgets."""
import math
import os
import re
import shutil
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import tsdf_restatement as TR                                  # noqa: E402
import tsdf_live_restatement as LR                             # noqa: E402
from go_slam_amd.tsdf_live import LiveFusion, ReversibleTSDF, plan_refresh      # noqa: E402

C = 2.013
TRUNC = 4 * TR.PLANE_VOXEL
STATE_KEYS = ("sum_s", "count", "sum_rgb", "count_rgb")


def same_state(a, b):
    return all(np.array_equal(a[k], b[k]) and a[k].dtype == np.int32 for k in STATE_KEYS)


@pytest.fixture(scope="module")
def plane():
    """The plane scene with random colours, fused once; the per-frame unquantised observations beside the state."""
    dims = TR.lattice_dims(TR.PLANE_BOUND, TR.PLANE_VOXEL)
    depth, w2c = TR.plane_scene(C)
    images = np.random.default_rng(11).random((3, 3) + TR.PLANE_HW, dtype=np.float32)
    obs = []
    state = LR.accumulate(LR.new_state(dims), depth, w2c, TR.PLANE_INTR, TR.PLANE_BOUND[:, 0], TR.PLANE_VOXEL, TRUNC,
                          images=images, observations=obs)
    return dims, depth, w2c, images, state, obs


def fuse(dims, depth, w2c, images, frames, sign=1, state=None):
    frames = list(frames)
    state = LR.new_state(dims) if state is None else state
    return LR.accumulate(state, depth[frames], w2c[frames], TR.PLANE_INTR, TR.PLANE_BOUND[:, 0], TR.PLANE_VOXEL, TRUNC,
                         images=images[frames], sign=sign)


def test_plane_count_is_the_number_of_cameras_that_see_the_point(plane):
    dims, _, _, _, state, _ = plane
    count, shaky = TR.plane_projection_counts(dims)
    z = (TR.PLANE_BOUND[2, 0] + np.arange(dims[2]) * TR.PLANE_VOXEL)[None, None, :] * np.ones(dims)
    front = C - z >= -TRUNC
    assert abs(C - z + TRUNC).min() > 1e-4                  # no lattice plane sits on the truncation boundary
    sel = front & ~shaky
    assert set(np.unique(count[sel])) == {0, 1, 2, 3}
    assert np.array_equal(state["count"][sel], count[sel].astype(np.int32))
    assert (state["count"][~front] == 0).all()


def test_resolved_values_are_the_fp64_mean_to_half_a_quantum(plane):
    dims, _, _, _, state, obs = plane
    n = int(np.prod(dims))
    s_sum, s_n, c_sum, c_n = np.zeros(n), np.zeros(n), np.zeros((3, n)), np.zeros(n)
    for sel, s, csel, col in obs:
        s_sum[sel] += s.astype(np.float64)
        s_n[sel] += 1
        c_sum[:, csel] += col.astype(np.float64)
        c_n[csel] += 1
    out = LR.resolve(state)
    seen, coloured = s_n > 0, c_n > 0
    assert seen.sum() > 0.2 * n and 0 < coloured.sum() < seen.sum()
    assert np.array_equal(out["weight"].reshape(-1), s_n.astype(np.float32))
    err = np.abs(out["tsdf"].reshape(-1).astype(np.float64)[seen] - s_sum[seen] / s_n[seen]).max()
    cerr = np.abs(out["colors"].reshape(3, -1).astype(np.float64)[:, coloured] - c_sum[:, coloured] / c_n[coloured]).max()
    print("max |tsdf - fp64 mean|:", err, "max |colour - fp64 mean|:", cerr)
    assert err <= 2.0 ** -15 + 2.0 ** -24                   # half a quantum of 1 / 16384, and the final rounding
    assert cerr <= 1.0 / 510.0 + 2.0 ** -24                 # half a quantum of 1 / 255, and the final rounding
    assert (out["tsdf"].reshape(-1)[~seen] == 1).all() and (out["colors"].reshape(3, -1)[:, ~coloured] == 0).all()


def test_linearity_and_order_independence(plane):
    dims, depth, w2c, images, state, _ = plane
    a_b = fuse(dims, depth, w2c, images, [0, 1])
    back = fuse(dims, depth, w2c, images, [0], sign=-1, state=a_b)            # +A +B -A
    assert same_state(back, fuse(dims, depth, w2c, images, [1]))
    assert same_state(fuse(dims, depth, w2c, images, [2, 0, 1]), state)
    mixed = LR.accumulate(LR.new_state(dims), depth[[0, 0, 1]], w2c[[0, 0, 1]], TR.PLANE_INTR, TR.PLANE_BOUND[:, 0],
                          TR.PLANE_VOXEL, TRUNC, images=images[[0, 0, 1]], sign=[1, -1, 1])
    assert same_state(mixed, fuse(dims, depth, w2c, images, [1]))
    gone = fuse(dims, depth, w2c, images, [1, 2, 0], sign=-1, state={k: v.copy() for k, v in state.items()})
    assert all(not gone[k].any() for k in STATE_KEYS)
    fresh = LR.resolve(gone)
    assert (fresh["tsdf"] == 1).all() and not fresh["weight"].any() and not fresh["colors"].any()


def _one_camera(depth_value, image_value=0.5, mask=None, sign=1):
    """tests/test_tsdf_cpu.py's lattice: 2 x 2 x 2 at x, y = +-0.125, z = 1 and 1.25 in front of an identity camera;
    trunc = 0.25."""
    depth = np.full((1, 8, 8), depth_value, np.float32)
    w2c = np.zeros((1, 3, 4), np.float32)
    w2c[0, :, :3] = np.eye(3)
    images = np.full((1, 3, 8, 8), image_value, np.float32)
    return LR.accumulate(LR.new_state((2, 2, 2)), depth, w2c, (8.0, 8.0, 3.5, 3.5), (-0.125, -0.125, 1.0), 0.25, 0.25,
                         images=images, mask=mask, sign=sign)


def test_truncation_boundary():
    at = _one_camera(1.0)                                   # z = 1.25: sdf == -trunc exactly, s = -1, q = -16384
    assert (at["sum_s"][:, :, 1] == -16384).all() and (at["count"][:, :, 1] == 1).all()
    assert (at["sum_s"][:, :, 0] == 0).all() and (at["count"][:, :, 0] == 1).all()
    assert (at["count_rgb"] == 1).all() and (at["sum_rgb"] == 128).all()      # rint(127.5) = 128, ties to even
    below = _one_camera(np.nextafter(np.float32(1.0), np.float32(0.0)))      # sdf one ulp under -trunc: skipped
    assert (below["count"][:, :, 1] == 0).all() and (below["sum_s"][:, :, 1] == 0).all()
    assert (below["count_rgb"][:, :, 1] == 0).all() and (below["count"][:, :, 0] == 1).all()


def test_just_above_trunc_updates_the_tsdf_and_not_the_colour():
    d = np.nextafter(np.float32(1.5), np.float32(2.0))      # z = 1.25: sdf one ulp above trunc; z = 1: far above
    st = _one_camera(d)
    assert np.float32(d) - np.float32(1.25) > np.float32(0.25)
    assert (st["sum_s"] == 16384).all() and (st["count"] == 1).all()
    assert not st["count_rgb"].any() and not st["sum_rgb"].any()
    at = _one_camera(1.5)                                   # sdf == trunc at z = 1.25: the colour is taken
    assert (at["count_rgb"][:, :, 1] == 1).all() and (at["count_rgb"][:, :, 0] == 0).all()
    out = LR.resolve(st)
    assert (out["tsdf"] == 1).all() and (out["weight"] == 1).all() and (out["colors"] == 0).all()


@pytest.mark.parametrize("value, want", [(np.nan, 0), (-0.3, 0), (1.7, 255), (np.inf, 255), (-np.inf, 0), (1.0, 255),
                                         (0.3, 76)])
def test_image_values_are_clamped_and_nan_is_black(value, want):
    st = _one_camera(1.1, image_value=value)
    assert (st["count_rgb"] == 1).all() and (st["sum_rgb"] == want).all()
    back = _one_camera(1.1, image_value=value, sign=-1)
    assert (back["sum_rgb"] == -want).all() and (back["count_rgb"] == -1).all() and (back["count"] == -1).all()
    assert (LR.resolve(back)["weight"] == 0).all() and (LR.resolve(back)["tsdf"] == 1).all()


def test_masked_and_zero_depth_pixels_leave_their_points_untouched():
    depth = np.full((1, 8, 8), 1.1, np.float32)
    mask = np.ones((1, 8, 8), np.float32)
    w2c = np.zeros((1, 3, 4), np.float32)
    w2c[0, :, :3] = np.eye(3)
    mask[0, 3, 3] = 0.0                                     # the pixels of tests/test_tsdf_cpu.py's case
    depth[0, 5, 5] = 0.0
    st = LR.accumulate(LR.new_state((2, 2, 2)), depth, w2c, (8.0, 8.0, 3.5, 3.5), (-0.125, -0.125, 1.0), 0.25, 0.25,
                       images=np.ones((1, 3, 8, 8), np.float32), mask=mask)
    assert (st["count"][0, 0] == 0).all() and (st["sum_s"][0, 0] == 0).all() and (st["count_rgb"][0, 0] == 0).all()
    assert st["count"][1, 1, 0] == 0 and st["count"][1, 1, 1] == 1 and st["count"][0, 1, 0] == 1
    # a masked pixel and the same pixel stored with depth 0 are the same observation: what LiveFusion's records rely on
    zeroed = np.where(mask == 0, np.float32(0), depth)
    st0 = LR.accumulate(LR.new_state((2, 2, 2)), zeroed, w2c, (8.0, 8.0, 3.5, 3.5), (-0.125, -0.125, 1.0), 0.25, 0.25,
                        images=np.ones((1, 3, 8, 8), np.float32))
    assert same_state(st, st0)


def test_frame_change_restated_against_fsum():
    g = np.random.default_rng(5)
    old = g.random((2, 5, 7), dtype=np.float32) + 0.5
    cur = old + g.normal(0, 0.01, old.shape).astype(np.float32)
    old[0, 1, 2] = 0.0
    cur[1, 4, 6] = -1.0
    m = np.zeros((2, 3, 4), np.float32)
    m[:, :, :3] = np.eye(3)
    m2 = m.copy()
    m2[0, :, 3] = (0.3, 0.0, 0.4)                           # the centre moves by 0.5, and so does every point
    out = LR.frame_change(old, cur, m, m2, 2.0)
    for f in range(2):
        both = (old[f] > 0) & (cur[f] > 0)
        assert out[f, 0] == both.sum() == 34
        want = math.fsum(float(v) for v in np.abs(cur[f] - old[f])[both])
        assert abs(out[f, 1] - want) <= 34 * 2.0 ** -52 * want
    assert abs(out[0, 2] - 0.5) < 1e-7 and abs(out[0, 3] - 0.5) < 1e-7 and out[1, 2] == 0 and out[1, 3] == 0
    assert (LR.frame_change(old, old, m2, m2, 2.0)[:, 1:] == 0).all()


# ---- plan_refresh ---------------------------------------------------------------------------------------------------
def test_plan_refresh_budget_threshold_age_ties_and_empty():
    assert plan_refresh([], [], 4, 0.1, 3) == ([], 0)
    scores = [0.05, 0.3, 0.1, 0.3, 0.2, 0.0]
    assert plan_refresh(scores, [0] * 6, 8, 0.1, 0) == ([1, 3, 4], 0)          # > threshold only, ties by lower index
    assert plan_refresh(scores, [0] * 6, 2, 0.1, 0) == ([1, 3], 1)             # the budget cuts, the rest is pending
    assert plan_refresh(scores, [0] * 6, 0, 0.1, 0) == ([], 3)
    assert plan_refresh(scores, [0] * 6, None, 0.0, 0) == ([1, 3, 4, 2, 0], 0)  # min_change 0 is exclusive
    ages = [5, 0, 9, 0, 0, 5]
    assert plan_refresh(scores, ages, 8, 0.1, 5) == ([1, 3, 4, 2, 0, 5], 0)    # then the stale ones, oldest first
    assert plan_refresh(scores, ages, 4, 0.1, 5) == ([1, 3, 4, 2], 2)
    assert plan_refresh(scores, ages, 8, 0.1, 0) == ([1, 3, 4], 0)             # max_age 0: age is ignored
    assert plan_refresh([0.2, float("nan")], [0, 0], 1, 0.1, 0) == ([1], 1)    # a pose that is no number goes first
    with pytest.raises(ValueError):
        plan_refresh([0.1], [], 1, 0.1, 0)


# ---- refusals that need no GPU --------------------------------------------------------------------------------------
BOUND = [[0, 1], [0, 1], [0, 1]]


def test_reversible_volume_keeps_the_lattice_rules():
    from go_slam_amd.tsdf import TSDFVolume
    vol = ReversibleTSDF(TR.PLANE_BOUND, TR.PLANE_VOXEL, device="cpu")
    ref = TSDFVolume(TR.PLANE_BOUND, TR.PLANE_VOXEL, device="cpu")
    assert vol.dims == ref.dims and vol.trunc == ref.trunc and np.array_equal(vol.lo, ref.lo)
    assert vol.sum_s.dtype == torch.int32 and tuple(vol.sum_rgb.shape) == (3,) + vol.dims and not vol.count.any()
    with pytest.raises(ValueError, match="axis y"):
        ReversibleTSDF([[0, 1], [0, 10.3], [0, 1]], 0.01, device="cpu")
    with pytest.raises(ValueError, match="empty"):
        ReversibleTSDF([[0, 1], [0, 1], [1, 0]], 0.1, device="cpu")
    with pytest.raises(ValueError, match="voxel_size"):
        ReversibleTSDF(BOUND, 0.0, device="cpu")
    with pytest.raises(ValueError, match="trunc"):
        ReversibleTSDF(BOUND, 0.1, trunc=-1.0, device="cpu")


def test_accumulate_refuses_before_the_device_is_touched(monkeypatch):
    from go_slam_amd import _lib
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was reached"))
    vol = ReversibleTSDF(BOUND, 0.25, device="cpu")
    depth, w2c, intr = torch.ones(2, 4, 4), torch.eye(4)[None].repeat(2, 1, 1), (4.0, 4.0, 1.5, 1.5)
    for sign in (0, 2, 0.5, True, "x", None, [1], [1, -1, 1], [1, 0], [1, 3]):
        with pytest.raises(ValueError, match="sign"):
            vol.accumulate(depth, w2c, intr, sign=sign)
    with pytest.raises(ValueError, match="depth must be"):
        vol.accumulate(torch.ones(4, 4), w2c, intr)
    with pytest.raises(ValueError, match="images must be"):
        vol.accumulate(depth, w2c, intr, images=torch.ones(2, 4, 4))
    with pytest.raises(ValueError, match="poses for"):
        vol.accumulate(depth, w2c[:1], intr)
    vol.n_live = 65534
    with pytest.raises(ValueError, match="65535"):
        vol.integrate(depth, w2c, intr)
    with pytest.raises(ValueError, match="65535"):
        vol.accumulate(depth.repeat(2, 1, 1), w2c.repeat(2, 1, 1), intr, sign=[1, 1, 1, -1])
    assert vol.n_live == 65534 and not vol.count.any()


def _stub_video(mode):
    return types.SimpleNamespace(disps_up=torch.zeros(4, 8, 8), cfg={"mode": mode}, counter=types.SimpleNamespace(value=2))


def test_live_fusion_refuses_the_filtered_source_and_sensor_without_depth():
    with pytest.raises(ValueError, match="filtered"):
        LiveFusion(_stub_video("rgbd"), BOUND, 0.25, source="filtered")
    with pytest.raises(ValueError, match="unknown source"):
        LiveFusion(_stub_video("rgbd"), BOUND, 0.25, source="depth")
    with pytest.raises(ValueError, match="sensor"):
        LiveFusion(_stub_video("mono"), BOUND, 0.25, source="sensor")
    with pytest.raises(ValueError, match="negative"):
        LiveFusion(_stub_video("rgbd"), BOUND, 0.25, budget=-1)
    live = LiveFusion(_stub_video("rgbd"), BOUND, 0.25)
    assert live.min_change == 0.125 and len(live) == 0 and tuple(live.rec_image.shape) == (4, 3, 8, 8)


def test_absent_or_disabled_key_builds_nothing():
    from go_slam_amd.tsdf_live import live_from_config
    for cfg in ({}, {"tsdf": None}, {"tsdf": {"enable": True}}, {"tsdf": {"enable": True, "live": {"enable": False}}}):
        assert live_from_config(types.SimpleNamespace(cfg=cfg)) is None


# ---- compiled resources ---------------------------------------------------------------------------------------------
def test_kernel_resources(tmp_path):
    """tests/test_abi.py's compile-only check for csrc/tsdf_live.hip: no kernel uses scratch, and the accumulate kernel
    stays within 64 VGPRs, the full 8 waves per SIMD its sibling tsdf_integrate_kernel runs at."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "go_slam_amd", "csrc")
    out = tmp_path / "k.s"
    res = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                          "-fno-gpu-rdc", "-munsafe-fp-atomics", "-I", csrc, "-I", os.path.join(ROOT, "include"),
                          "--cuda-device-only", "-S", os.path.join(csrc, "tsdf_live.hip"), "-o", str(out)],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-2000:]
    pat = re.compile(r"\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.name:\s+(\S+)\n(?:.*\n)*?"
                     r"\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)")
    seen = {}
    for m in pat.finditer(open(out).read()):
        lds, name, scratch, vgpr = int(m.group(1)), m.group(2), int(m.group(3)), int(m.group(4))
        print(name, "VGPRs", vgpr, "LDS", lds, "scratch", scratch)
        assert scratch == 0, f"{name}: {scratch} B of scratch"
        for key in ("tsdf_accumulate_kernel", "tsdf_resolve_kernel", "tsdf_frame_change_kernel"):
            if key in name:
                seen[key] = seen.get(key, 0) + 1
        if "tsdf_accumulate_kernel" in name:
            assert vgpr <= 64 and lds == 0, f"{name}: {vgpr} VGPRs, {lds} B of LDS"
    assert seen == {"tsdf_accumulate_kernel": 2, "tsdf_resolve_kernel": 2, "tsdf_frame_change_kernel": 1}, seen
