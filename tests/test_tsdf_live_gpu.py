"""Reversible TSDF fusion on the MI355X (csrc/tsdf_live.hip, go_slam_amd/tsdf_live.py): the integer state equals the
serial restatement (tests/tsdf_live_restatement.py) bit for bit; taking frames out, permuting them, cutting the calls and
mixing signs in one call all end in the state of a fresh fusion of the surviving observations; the resolved volume is the
restated one and within half a quantum of the running-mean fusion; LiveFusion follows a video whose poses, depths and
keyframe slots change; and a whole only-tracking run ends with a live volume equal to a fresh fusion of its final video."""
import math
import os
import random
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from go_slam_amd import synth                                  # noqa: E402
import tsdf_live_restatement as LR                             # noqa: E402
import test_tsdf_gpu as TG                                     # noqa: E402  (its lattice, frames, video and whole run)
from test_tsdf_gpu import arc_frames                           # noqa: E402,F401  (the fixture)

pytestmark = pytest.mark.gpu
DEV = TG.DEV
DIMS, LO = (37, 21, 70), [b[0] for b in TG.BOUND_EXACT]
VOXEL, TRUNC, INTR = TG.VOXEL, 4 * TG.VOXEL, TG.INTR
KEYS = ("sum_s", "count", "sum_rgb", "count_rgb")
OUT = {1, 4, 16, 17, 32}


def live_volume(bound=TG.BOUND_EXACT, voxel=VOXEL):
    from go_slam_amd.tsdf_live import ReversibleTSDF
    return ReversibleTSDF(bound, voxel, device=DEV)


def host(vol):
    return {k: t.cpu().numpy() for k, t in zip(KEYS, vol.state())}


def assert_state(vol, ref, color=True):
    got = host(vol)
    for k in KEYS if color else KEYS[:2]:
        assert got[k].dtype == np.int32 and np.array_equal(got[k], ref[k]), k


def assert_same(a, b):
    for x, y in zip(a.state(), b.state()):
        assert torch.equal(x, y)


def pick(frames, idx):
    idx = list(idx)
    return tuple(a[idx] for a in frames)


def accumulate(vol, frames, sign=1, images=True):
    depth, mats, img, mask = frames
    vol.accumulate(torch.from_numpy(depth), torch.from_numpy(mats), INTR, images=torch.from_numpy(img) if images else None,
                   mask=torch.from_numpy(mask), sign=sign)
    return vol


def restate(frames, sign=1, images=True, state=None):
    depth, mats, img, mask = frames
    state = LR.new_state(DIMS) if state is None else state
    return LR.accumulate(state, depth, mats, INTR, LO, VOXEL, TRUNC, images=img if images else None, mask=mask, sign=sign)


@pytest.fixture(scope="module")
def arc_reference(arc_frames):
    return restate(arc_frames)


def test_accumulate_is_the_restatement_bit_for_bit(arc_frames, arc_reference):
    vol = live_volume()
    assert vol.dims == DIMS and vol.trunc == TRUNC
    accumulate(vol, arc_frames)
    ref = arc_reference
    seen = ref["count"] > 0
    print("share of points updated:", seen.mean(), "largest count:", ref["count"].max(), "coloured:", (ref["count_rgb"] > 0).mean())
    assert 0.05 < seen.mean() < 0.9 and ref["count"].max() > TG.batch() and (ref["count_rgb"] < ref["count"]).any()
    assert_state(vol, ref)
    assert vol.n_live == len(arc_frames[0])
    plain = accumulate(live_volume(), arc_frames, images=False)
    assert_state(plain, ref, color=False)
    assert not bool(plain.sum_rgb.any()) and not bool(plain.count_rgb.any())
    vol.reset()
    assert vol.n_live == 0 and not any(bool(t.any()) for t in vol.state())


@pytest.mark.parametrize("images", [True, False])
def test_both_fusions_count_the_same_observations(arc_frames, arc_reference, images):
    """The running mean and the integer sums are one sweep with two rules: with no weight cap in reach, a point's weight
    and its count are the number of frames that update it, the restatement's."""
    K = len(arc_frames[0])
    mean = TG.integrate(TG.volume(max_weight=64.0), arc_frames, images=images)
    rev = accumulate(live_volume(), arc_frames, images=images)
    want = arc_reference["count"]
    assert K <= 64 and want.max() > TG.batch() and (want == 0).any()
    assert np.array_equal(TG.bits(mean.weight), TG.bits(rev.count.float()))
    assert np.array_equal(TG.bits(mean.weight), TG.bits(want.astype(np.float32)))
    assert np.array_equal(rev.count.cpu().numpy(), want)


SMALL_BOUND = [[0.75, 1.0], [0.5, 0.625], [-2.0, 6.0]]         # 3 x 2 x 65 at VOXEL: a second 64-point run of one point


def test_a_lattice_one_point_longer_than_a_run_is_the_restatement(arc_frames):
    """batch + 1 frames, so a second launch of one frame, on the smallest lattice with a ragged second run and ny = 2:
    arc frames, which see the first run only, a camera at z = 5.99 that has nothing but the plane k = 64 in front of it,
    one at z = 4 that sees both runs and one that looks away.  accumulate takes them with mixed signs."""
    dims, lo = (3, 2, 65), [b[0] for b in SMALL_BOUND]
    arc = list(range(0, len(arc_frames[0]), 2))[:TG.batch() - 2]
    parts = [pick(arc_frames, arc[:5]), TG.one_frame(np.eye(3), (0.875, 0.5, 5.99), 0.3), pick(arc_frames, arc[5:10]),
             TG.one_frame(np.eye(3), (0.875, 0.5625, 4.0), 2.0),
             TG.one_frame(np.diag([-1.0, 1.0, -1.0]), (0.75, 0.5, -3.0), 2.0), pick(arc_frames, arc[10:])]
    frames = tuple(np.concatenate([p[i] for p in parts]) for i in range(4))
    depth, mats, img, mask = frames
    K = len(depth)
    assert K == TG.batch() + 1 and not mask.all() and not depth.all()
    signs = [1, 1, -1, 1, 1, 1, -1, 1, 1, 1, 1, -1, -1, 1, -1, 1, -1]
    # not vacuous: some points are updated and some are not, the spilled plane is, and one frame updates nothing else
    ref = TG.restate(frames, dims, lo, VOXEL, TRUNC)
    touched = ref["weight"] > 0
    alone = TG.restate(pick(frames, [5]), dims, lo, VOXEL, TRUNC)["weight"] > 0
    print("points touched:", int(touched.sum()), "of", touched.size, "on k = 64:", int(touched[:, :, 64].sum()))
    assert 0 < touched.sum() < touched.size and touched[:, :, 64].any() and (ref["colors"] > 0).any()
    assert alone[:, :, 64].any() and not alone[:, :, :64].any()
    vol = TG.integrate(TG.volume(SMALL_BOUND), frames)
    assert vol.dims == dims
    TG.assert_state(vol, ref)
    state = LR.accumulate(LR.new_state(dims), depth, mats, INTR, lo, VOXEL, TRUNC, images=img, mask=mask, sign=signs)
    assert len(set(signs[:TG.batch()])) == 2 and state["count"].min() < 0 < state["count"].max()
    rev = accumulate(live_volume(SMALL_BOUND), frames, sign=signs)
    assert rev.dims == dims and rev.n_live == sum(signs)
    assert_state(rev, state)


def test_frames_taken_out_leave_a_fresh_fusion_of_the_rest(arc_frames, arc_reference):
    K = len(arc_frames[0])
    rest = [f for f in range(K) if f not in OUT]
    vol = accumulate(live_volume(), arc_frames)
    accumulate(vol, pick(arc_frames, sorted(OUT)), sign=-1)
    assert vol.n_live == K - len(OUT)
    ref = restate(pick(arc_frames, rest))
    assert any(not np.array_equal(ref[k], arc_reference[k]) for k in KEYS)
    assert_state(vol, ref)
    assert_same(vol, accumulate(live_volume(), pick(arc_frames, rest)))


def test_a_permutation_cut_at_an_odd_frame_gives_the_same_bits(arc_frames, arc_reference):
    K = len(arc_frames[0])
    perm = np.random.default_rng(3).permutation(K).tolist()
    assert perm != sorted(perm)
    vol = live_volume()
    accumulate(vol, pick(arc_frames, perm[:7]))
    accumulate(vol, pick(arc_frames, perm[7:]))
    assert_state(vol, arc_reference)


def perturbed(mats, seed=9):
    """The matrices moved by a few centimetres and degrees: (dR R | dR t + dt), rounded once."""
    g = np.random.default_rng(seed)
    out = np.empty_like(mats)
    for f, m in enumerate(mats):
        ax = g.normal(size=3)
        ax /= np.linalg.norm(ax)
        a = math.radians(g.uniform(1.0, 3.0))
        Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
        dR = np.eye(3) + math.sin(a) * Kx + (1 - math.cos(a)) * Kx @ Kx
        out[f, :, :3] = dR @ m[:, :3].astype(np.float64)
        out[f, :, 3] = dR @ m[:, 3].astype(np.float64) + g.uniform(-0.05, 0.05, 3)
    return out


def test_mixed_signs_in_one_call_move_every_frame(arc_frames):
    depth, mats, img, mask = arc_frames
    K = len(depth)
    moved = perturbed(mats)
    vol = accumulate(live_volume(), arc_frames)
    two = lambda a, b: np.stack([a, b], axis=1).reshape((2 * K,) + a.shape[1:])       # noqa: E731  (interleaved)
    accumulate(vol, (two(depth, depth), two(mats, moved), two(img, img), two(mask, mask)), sign=[-1, 1] * K)
    assert vol.n_live == K
    new_frames = (depth, moved, img, mask)
    fresh = accumulate(live_volume(), new_frames)
    assert not torch.equal(fresh.sum_s, accumulate(live_volume(), arc_frames).sum_s)
    assert_same(vol, fresh)
    assert_state(vol, restate(new_frames))


def test_taking_everything_out_leaves_a_fresh_volume(arc_frames):
    from go_slam_amd.tsdf import TSDFVolume
    vol = accumulate(live_volume(), arc_frames)
    half = vol.resolve()
    assert float(half.weight.max()) > 1
    accumulate(vol, pick(arc_frames, range(len(arc_frames[0]) - 1, -1, -1)), sign=-1)
    assert vol.n_live == 0 and not any(bool(t.any()) for t in vol.state())
    out, fresh = vol.resolve(), TSDFVolume(TG.BOUND_EXACT, VOXEL, device=DEV)
    TG.assert_same_volume(out, fresh)


def test_resolve_is_the_restatement_and_close_to_the_running_mean(arc_frames, arc_reference):
    K = len(arc_frames[0])
    vol = accumulate(live_volume(), arc_frames)
    out = vol.resolve()
    assert vol.resolve() is out                             # kept until the state changes
    ref = LR.resolve(arc_reference)
    for name in ("tsdf", "weight", "colors"):
        assert np.array_equal(TG.bits(getattr(out, name)), TG.bits(ref[name])), name
    mean = TG.integrate(TG.volume(max_weight=64.0), arc_frames)
    assert K <= 64 and torch.equal(mean.weight, out.weight)
    seen = out.weight > 0
    err = float((out.tsdf.double() - mean.tsdf.double()).abs()[seen].max())
    bound = 2.0 ** -15 + (K + 1) * 2.0 ** -23               # half a quantum, and one rounding per running-mean step
    print(f"max |resolved - running mean| over {int(seen.sum())} points: {err:.3e} (bound {bound:.3e})")
    assert err <= bound
    assert torch.equal(out.tsdf[~seen], mean.tsdf[~seen])
    mesh = out.extract_mesh()
    assert len(mesh.faces) > 100 and len(mesh.vertex_colors) == len(mesh.vertices)
    flags_before = out.brick_flags()
    cast = out.raycast(torch.from_numpy(arc_frames[1][:1]), INTR, (TG.H, TG.W))
    assert int((cast["depth"] > 0).sum()) > 100 and cast["color"] is not None
    field = out.esdf(max_distance=1.0)
    assert int((field.state == 2).sum()) > 0 and bool(torch.isfinite(field.dist).all())
    accumulate(vol, pick(arc_frames, [0]), sign=-1)         # the cache and its brick flags go with the state
    again = vol.resolve()
    assert again._flags is None and again.brick_flags() is not flags_before
    assert not torch.equal(again.weight, mean.weight)


def test_a_frame_that_looks_away_changes_nothing_and_a_corner_is_the_restatement(arc_frames, arc_reference):
    vol = accumulate(live_volume(), arc_frames)
    away = TG.one_frame(np.diag([-1.0, 1.0, -1.0]), (0.75, 0.5, -3.0), 2.0)
    accumulate(vol, away)
    assert_state(vol, arc_reference)
    assert_state(vol, restate(away, state={k: v.copy() for k, v in arc_reference.items()}))
    corner = TG.one_frame(np.eye(3), (2.6, 1.4, 5.5), 0.8)
    ref = restate(corner)
    touched = ref["count"] > 0
    assert 0 < touched.sum() < 0.02 * touched.size
    assert_state(accumulate(live_volume(), corner), ref)


def test_bad_arguments_are_refused_before_any_launch(built_lib):
    from go_slam_amd import _lib
    L = _lib.lib()
    x = torch.full((64,), 7, dtype=torch.int32, device=DEV)
    f = torch.full((64,), 7.0, device=DEV)
    P, S = _lib.ptr, _lib.stream_ptr(DEV)

    def acc(state=(x, x, x, x), dims=(2, 2, 2), depth=f, images=None, w2c=f, sign=x, k=1, hw=(2, 2), fx=1.0, fy=1.0,
            voxel=0.1, trunc=0.4):
        return L.gs_tsdf_accumulate(*(P(t) for t in state), *dims, P(depth), None, P(images), P(w2c), P(sign), k, *hw,
                                    fx, fy, 0.5, 0.5, 0.0, 0.0, 0.0, voxel, trunc, S)

    for dims in [(1, 2, 2), (2, 1025, 2), (2, 2, 0)]:
        assert acc(dims=dims) == -1 and b"outside [2, 1024]" in L.gs_last_error()
        assert L.gs_tsdf_resolve(P(x), P(x), P(x), P(x), *dims, P(f), P(f), P(f), S) == -1
    assert acc(state=(None, x, x, x)) == -1 and acc(state=(x, None, x, x)) == -1
    assert acc(depth=None) == -1 and acc(w2c=None) == -1 and acc(sign=None) == -1
    assert acc(state=(x, x, None, x), images=f) == -1 and acc(state=(x, x, x, None), images=f) == -1
    assert acc(fx=0.0) == -1 and acc(fy=-1.0) == -1 and acc(voxel=0.0) == -1 and acc(trunc=0.0) == -1
    assert acc(k=-1) == -1 and acc(hw=(0, 2)) == -1
    assert acc(k=0) == 0 and acc(state=(x, x, None, None), k=0) == 0
    assert L.gs_tsdf_resolve(P(x), P(x), None, P(x), 2, 2, 2, P(f), P(f), P(f), S) == -1
    assert L.gs_tsdf_resolve(P(x), P(x), P(x), P(x), 2, 2, 2, P(f), P(f), None, S) == -1
    assert L.gs_tsdf_resolve(P(x), None, None, None, 2, 2, 2, P(f), P(f), None, S) == -1
    assert L.gs_tsdf_frame_change(P(f), P(f), P(f), None, 1, 2, 2, 2.0, P(f), S) == -1
    assert L.gs_tsdf_frame_change(P(f), P(f), P(f), P(f), 1, 0, 2, 2.0, P(f), S) == -1
    assert L.gs_tsdf_frame_change(None, None, None, None, 0, 2, 2, 2.0, None, S) == 0      # k == 0 launches nothing
    torch.cuda.synchronize()
    assert bool((x == 7).all()) and bool((f == 7.0).all())


@pytest.mark.parametrize("h, w", [(48, 64), (5, 7), (1, 1)])
def test_frame_change(built_lib, arc_frames, h, w):
    from go_slam_amd import _lib
    g = torch.Generator().manual_seed(h * w)
    k = 3
    old = torch.rand(k, h, w, generator=g) * 3 + 0.5
    cur = old + 0.02 * torch.randn(k, h, w, generator=g)
    old[torch.rand(k, h, w, generator=g) < 0.2] = 0.0
    cur[torch.rand(k, h, w, generator=g) < 0.1] = -1.0
    m_old = arc_frames[1][[0, 5, 9]]
    m_new = perturbed(m_old, seed=2)
    m_new[1] = m_old[1]

    def run(a, b, ma, mb, n=k):
        out = torch.full((k, 4), -1.0, dtype=torch.float64, device=DEV)
        dev = [a.to(DEV), b.to(DEV), torch.from_numpy(ma).to(DEV), torch.from_numpy(mb).to(DEV)]       # alive over the call
        rc = _lib.lib().gs_tsdf_frame_change(*(_lib.ptr(t) for t in dev), n, h, w, 2.0, _lib.ptr(out), _lib.stream_ptr(DEV))
        assert rc == 0
        return out.cpu().numpy()

    out = run(old, cur, m_old, m_new)
    assert np.array_equal(out, run(old, cur, m_old, m_new))                 # two runs agree bitwise
    ref = LR.frame_change(old.numpy(), cur.numpy(), m_old, m_new, 2.0)
    assert np.array_equal(out[:, :2], ref[:, :2])                           # the sums in the header's order: the same bits
    assert np.allclose(out[:, 2:], ref[:, 2:], rtol=1e-14, atol=0)
    for f in range(k):
        both = (old[f] > 0) & (cur[f] > 0)
        n = int(both.sum())
        assert out[f, 0] == n
        want = math.fsum((cur[f] - old[f]).abs()[both].tolist())
        assert abs(out[f, 1] - want) <= n * 2.0 ** -52 * want
        for col, ref in ((2, 0.0), (3, 2.0)):
            pts = []
            for m in (m_old[f], m_new[f]):
                R, t = m[:, :3].astype(np.float64), m[:, 3].astype(np.float64)
                pts.append(R.T @ (np.array([0.0, 0.0, ref]) - t))
            want = np.linalg.norm(pts[1] - pts[0])
            assert abs(out[f, col] - want) <= 1e-12 * (1 + np.linalg.norm(m_new[f][:, 3])), (f, col)
    assert out[1, 2] == 0 and out[1, 3] == 0 and out[0, 2] > 0 and out[2, 3] > 0
    same = run(old, old, m_old, m_old)
    assert (same[:, 1:] == 0).all() and (same[:, 0] == (old > 0).sum(dim=(1, 2)).numpy()).all()
    assert (run(old, cur, m_old, m_new, n=0) == -1).all()                   # k == 0: nothing is written


# ---- LiveFusion -----------------------------------------------------------------------------------------------------
def fresh_fusion(video, source, bound, voxel):
    """A fresh ReversibleTSDF of the video as it stands, through fuse_keyframes' rule with the restated mask count."""
    import pointcloud_restatement as R
    from go_slam_amd.lietorch_shim import SE3
    from go_slam_amd.tsdf import keyframe_observations
    ids = torch.arange(int(video.counter.value))
    intr = (video.intrinsics[0] * 8).contiguous()
    w2w_inv = SE3(video.pose_compensate[0].clone().unsqueeze(0)).inv()
    depth, w2c, images, mask = keyframe_observations(
        video, source, ids, intr, w2w_inv, 0.01, 2,
        depth_filter=lambda poses, disps, k, index, thresh: R.tracked_counts(poses, disps, k, index, 0.01))
    return live_volume(bound, voxel).integrate(depth, w2c, intr.cpu().tolist(), images=images, mask=mask)


def remove_keyframe(video, ix):
    """What the frontend's rm_keyframe and counter decrement do to the buffers: the slots above move down by one."""
    from go_slam_amd.factor_graph import FactorGraph
    n = int(video.counter.value)
    for name in FactorGraph._KEYFRAME_BUFFERS:
        buf = getattr(video, name, None)
        if torch.is_tensor(buf):
            buf[ix:n - 1] = buf[ix + 1:n].clone()
    video.counter = n - 1


def until_settled(live, limit=12):
    calls = []
    for _ in range(limit):
        calls.append(live.update())
        if calls[-1]["pending"] == 0:
            return calls
    raise AssertionError(f"still pending after {limit} updates: {calls}")


@pytest.mark.parametrize("source", ["tracked", "sensor"])
def test_live_fusion_follows_the_video(built_lib, source):
    from go_slam_amd.tsdf_live import LiveFusion
    v = TG.make_video(12, 16)
    v.timestamp[:12] = torch.arange(12, device=DEV) * 3.0
    if source == "sensor":
        v.depths_gt[:12] = TG.inverse(v.disps_up[:12])
    live = LiveFusion(v, TG.BOUND_VIDEO, 0.1, source=source, budget=2)
    first = until_settled(live)
    assert first[0] == {"integrated": 11, "refused": 0, "removed": 0, "pending": 0} and len(live) == 11       # lag 1
    assert live.volume_state.n_live == 11 and float(live.volume().weight.max()) > 1
    v.poses[[2, 6, 9], :3] += torch.tensor([[0.07, 0.0, 0.02], [0.0, -0.08, 0.0], [0.03, 0.03, 0.06]], device=DEV)
    v.disps_up[[3, 8]] *= 1.02
    if source == "sensor":
        v.depths_gt[[3, 8]] /= 1.02
    remove_keyframe(v, 5)
    calls = until_settled(live)
    print(source, "updates after the change:", calls)
    assert all(c["refused"] <= 2 for c in calls) and len(calls) >= 2 and calls[0]["pending"] > 0
    assert calls[0]["removed"] == 1 and sum(c["removed"] for c in calls) == 1
    assert sum(c["refused"] for c in calls) >= 3 and len(live) == 10
    last = live.finish()
    print(source, "finish:", last)
    assert last["integrated"] == 1 and len(live) == 11 == live.volume_state.n_live
    assert_same(live.volume_state, fresh_fusion(v, source, TG.BOUND_VIDEO, 0.1))
    assert live.update() == {"integrated": 0, "refused": 0, "removed": 0, "pending": 0}
    assert len(live.mesh().faces) > 100


# ---- a whole run ----------------------------------------------------------------------------------------------------
def whole_run(out_dir, tsdf_cfg):
    """tests/test_tsdf_gpu.py's whole_run, keeping terminate's statistics."""
    from go_slam_amd.slam import SLAM
    torch.manual_seed(43)
    torch.cuda.manual_seed_all(43)
    np.random.seed(43)
    random.seed(43)
    cfg = TG.make_cfg(out_dir, True)
    cfg["tsdf"] = tsdf_cfg
    args = types.SimpleNamespace(device="cuda:0", make_video=False, output=None)
    slam = SLAM(args, cfg, full_ba_every=4)
    with torch.no_grad():
        slam.net.update.delta[2].weight.mul_(0.02)
        slam.net.update.delta[2].bias.zero_()
    slam.ba.frontend_window = 8
    N, H, W = TG.N_RUN, TG.H_RUN, TG.W_RUN
    stream = synth.PlaneSequence(N, H, W, 0.9 * W, 0.9 * W, W / 2 - 0.5, H / 2 - 0.5)
    slam.run(stream)
    stats = slam.terminate(rank=-1, stream=stream)
    torch.cuda.synchronize()
    return slam, stats


def test_only_tracking_run_keeps_a_live_volume(built_lib, tmp_path):
    from go_slam_amd import tsdf
    from go_slam_amd.neus.mesh import load_mesh
    base = {"enable": True, "source": "sensor", "voxel_size": 0.1}
    with_dir, without_dir = str(tmp_path / "with"), str(tmp_path / "without")
    slam, stats = whole_run(with_dir, dict(base, live={"enable": True, "budget": 2, "mesh_every": 4}))
    n_kf = int(slam.video.counter.value)
    files = TG.listing(with_dir)
    previews = [p for p in files if p.startswith(os.path.join("mesh", "live") + os.sep)]
    print("keyframes:", n_kf, "re-fused over the run:", stats["tsdf_live_refused"], "previews:", previews)
    assert os.path.join("mesh", "tsdf_live_mesh.ply") in files and len(previews) >= 1
    assert all(p.endswith(".ply") and int(os.path.basename(p)[:5]) % 4 == 0 for p in previews)
    assert stats["tsdf_live_keyframes"] == n_kf == len(slam.live) and stats["tsdf_live_refused"] >= 0
    mesh = load_mesh(f"{with_dir}/mesh/tsdf_live_mesh.ply")
    assert len(mesh.faces) >= 1 and mesh.vertex_colors is not None
    bound = slam.cfg["mapping"]["bound"]
    assert_same(slam.live.volume_state, fresh_fusion(slam.video, "sensor", bound, 0.1))
    vol, _ = tsdf.fuse_keyframes(slam.video, bound, 0.1, source="sensor")     # what fuse_from_config built in terminate
    out = slam.live.volume()
    assert n_kf <= 64 and torch.equal(out.weight, vol.weight)
    seen = out.weight > 0
    err = float((out.tsdf.double() - vol.tsdf.double()).abs()[seen].max())
    bnd = 2.0 ** -15 + (n_kf + 1) * 2.0 ** -23
    print(f"max |live - fuse_keyframes| over {int(seen.sum())} points: {err:.3e} (bound {bnd:.3e})")
    assert int(seen.sum()) > 1000 and err <= bnd
    plain, plain_stats = whole_run(without_dir, dict(base))
    assert plain.live is None and not any(k.startswith("tsdf_live") for k in plain_stats)
    assert [p for p in files if p not in previews and p != os.path.join("mesh", "tsdf_live_mesh.ply")] == TG.listing(without_dir)
    assert np.array_equal(np.load(f"{with_dir}/checkpoints/est_poses.npy"), np.load(f"{without_dir}/checkpoints/est_poses.npy"))
    assert open(f"{with_dir}/mesh/tsdf_mesh.ply", "rb").read() == open(f"{without_dir}/mesh/tsdf_mesh.ply", "rb").read()
