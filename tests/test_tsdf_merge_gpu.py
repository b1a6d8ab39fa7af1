"""Volume-to-volume registration and merge on the MI355X (csrc/tsdf_merge.hip, go_slam_amd/tsdf_merge.py): the
Gauss-Newton rows, a whole `register` with its trace, and the merged lattices equal tests/tsdf_merge_restatement.py bit
for bit (integer views) at every stride, across chunk boundaries, with and without colours and for every input the
contract names; skipped points keep their bits; bad arguments are refused without a write; and a second only-tracking
rgbd run with tsdf.merge joins its volume with the first run's saved one."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from go_slam_amd import synth                                  # noqa: E402
import test_tsdf_gpu as TG                                     # noqa: E402  (its lattice, frames and whole run)
import tsdf_align_restatement as AR                            # noqa: E402
import tsdf_merge_restatement as MR                            # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W = TG.H, TG.W
GUARD = 64                                                     # elements of padding on each side of a guarded buffer
S_VOXEL = 0.15625                                              # 1.25 x TG.VOXEL, exact in binary
S_BOUND = [[-1.625, 3.0625], [-1.0, 1.8125], [-0.5, 5.59375]]  # 31 x 19 x 40 at S_VOXEL, in S's world
LEVELS = ((2, 10), (1, 10))


def s_to_d():
    """The true transform S-world to D-world: 3 cm and 1.5 degrees."""
    eye = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)
    return AR.displaced(eye, 0.03, 1.5, np.random.default_rng(17))


def four(m):
    out = np.eye(4)
    out[:3, :] = np.asarray(m, np.float64)[:3, :]
    return out


def arc_inputs(K):
    """TG.arc_frames' frames: (depth, w2c float32 [K,3,4], images, mask), and the same poses for S's world: a camera
    that sees x_D = T x_S has the world-to-camera matrix W T, formed in float64 and rounded once."""
    from go_slam_amd.tsdf import w2c_matrices
    poses = synth.arc_poses(K)
    disp = synth.plane_disps(poses, torch.tensor(TG.INTR), H, W)
    depth = torch.where(disp > 0, 1.0 / disp, torch.zeros_like(disp))
    g = torch.Generator().manual_seed(7)
    depth[torch.rand(K, H, W, generator=g) < 0.05] = 0.0
    mask = (torch.rand(K, H, W, generator=g) > 0.2).float()
    images = torch.rand(K, 3, H, W, generator=g)
    w2c = w2c_matrices(poses).numpy()
    T = four(s_to_d())
    w2c_s = np.stack([(four(m) @ T)[:3, :] for m in w2c]).astype(np.float32)
    return depth.numpy(), w2c, images.numpy(), mask.numpy(), w2c_s


def as_dict(vol, colors=True):
    return MR.volume(vol.tsdf.cpu().numpy(), vol.weight.cpu().numpy(), vol.lo, vol.voxel, vol.trunc,
                     vol.colors.cpu().numpy() if colors else None)


def copy_of(vol):
    from go_slam_amd.tsdf import TSDFVolume
    out = TSDFVolume.__new__(TSDFVolume)
    out.voxel, out.lo, out.dims, out.trunc, out.max_weight, out.device = vol.voxel, vol.lo.copy(), vol.dims, vol.trunc, \
        vol.max_weight, vol.device
    out.tsdf, out.weight, out.colors, out._flags = vol.tsdf.clone(), vol.weight.clone(), vol.colors.clone(), None
    return out


def from_dict(d, max_weight=64.0):
    from go_slam_amd.tsdf import TSDFVolume
    out = TSDFVolume.__new__(TSDFVolume)
    out.voxel, out.lo, out.dims, out.trunc, out.max_weight = d["voxel"], np.asarray(d["lo"], np.float64), d["tsdf"].shape, \
        d["trunc"], max_weight
    out.device = torch.device(DEV)
    out.tsdf, out.weight = torch.from_numpy(d["tsdf"]).to(DEV), torch.from_numpy(d["weight"]).to(DEV)
    out.colors = torch.from_numpy(d["colors"]).to(DEV) if "colors" in d else torch.zeros((3,) + d["tsdf"].shape, device=DEV)
    out._flags = None
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def same_state(vol, ref, colors=True):
    ok = np.array_equal(TG.bits(vol.tsdf), TG.bits(ref["tsdf"])) and np.array_equal(TG.bits(vol.weight), TG.bits(ref["weight"]))
    return ok and (not colors or np.array_equal(TG.bits(vol.colors), TG.bits(ref["colors"])))


def chunk():
    from go_slam_amd import _lib
    return int(_lib.lib().gs_tsdf_align_chunk())


def lattice_args(vol):
    return [*vol.dims, float(vol.lo[0]), float(vol.lo[1]), float(vol.lo[2]), vol.voxel, vol.trunc]


def raw_system(dst, src, pose, stride, min_weight=1.0, huber=0.5):
    """gs_tsdf_register_system through ctypes on fresh buffers -> (rc, rows [B,32] host)."""
    from go_slam_amd import _lib
    L = _lib.lib()
    pose = np.asarray(pose, np.float64).reshape(-1, 3, 4)
    B = pose.shape[0]
    pose_d = torch.as_tensor(pose).to(DEV).contiguous()
    ws = torch.empty(max(L.gs_tsdf_register_workspace_bytes(B, *src.dims, stride) // 8, 1), dtype=torch.float64, device=DEV)
    out = torch.full((B, 32), 7.0, dtype=torch.float64, device=DEV)
    rc = L.gs_tsdf_register_system(_lib.ptr(dst.tsdf), _lib.ptr(dst.weight), *lattice_args(dst), _lib.ptr(src.tsdf),
                                   _lib.ptr(src.weight), *lattice_args(src), _lib.ptr(pose_d), B, stride, min_weight, huber,
                                   _lib.ptr(ws), _lib.ptr(out), _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()


@pytest.fixture(scope="module")
def scene(built_lib):
    """D: test_tsdf_gpu.py's 37 x 21 x 70 lattice fused on the GPU from all its arc frames (5 % zero depth, a random
    mask: real weights and unseen cells).  S: 31 x 19 x 40 at 1.25 times the voxel (truncation 0.625 m against 0.5 m),
    fused from every second frame with poses composed with the true transform, so S's world is 3 cm / 1.5 degrees off
    D's.  Eight transforms: the truth, six displaced ones and one that carries S out of D."""
    from go_slam_amd.tsdf import TSDFVolume
    K = 2 * TG.batch() + 1
    depth, w2c, images, mask, w2c_s = arc_inputs(K)
    D = TG.volume()
    assert D.dims == (37, 21, 70)
    D.integrate(torch.from_numpy(depth), torch.from_numpy(w2c), TG.INTR, images=torch.from_numpy(images),
                mask=torch.from_numpy(mask))
    S = TSDFVolume(S_BOUND, S_VOXEL, device=DEV)
    assert S.dims == (31, 19, 40) and S.trunc == 0.625
    sl = slice(1, None, 2)
    S.integrate(torch.from_numpy(depth[sl]), torch.from_numpy(w2c_s[sl]), TG.INTR, images=torch.from_numpy(images[sl]),
                mask=torch.from_numpy(mask[sl]))
    T = s_to_d()
    rng = np.random.default_rng(19)
    poses = np.stack([T] + [AR.displaced(T, m, d, rng) for m, d in ((0.02, 1.0), (0.05, 3.0), (0.1, 5.0), (0.03, 0.0),
                                                                     (0.0, 2.0), (0.2, 10.0))]
                     + [np.concatenate([T[:, :3], (T[:, 3] + [40.0, 0.0, 0.0])[:, None]], 1)])
    return {"D": D, "S": S, "d": as_dict(D), "s": as_dict(S), "T": T, "poses": poses}


@pytest.mark.parametrize("stride", [1, 2, 3, 5])
def test_rows_equal_the_restatement_bit_for_bit(scene, stride):
    """Eight hypotheses in one launch, the first of them alone, and both a second time: equal bits.  31 * 19 * 40 = 23560
    samples at stride 1 are a dozen chunks."""
    ref = MR.system(scene["d"], scene["s"], scene["poses"], stride, chunk())
    print("count per transform:", ref[:, 28], "considered:", ref[:, 30])
    assert (ref[:7, 28] > 0).all() and (ref[:7, 28] < ref[:7, 30]).all() and ref[7, 28] == 0 and ref[7, 30] == ref[0, 30]
    assert (ref[:, 31] == 0).all()
    rc, out = raw_system(scene["D"], scene["S"], scene["poses"], stride)
    assert rc == 0 and same_bits(out, ref)
    rc, one = raw_system(scene["D"], scene["S"], scene["poses"][:1], stride)
    assert rc == 0 and same_bits(one, ref[:1])
    assert same_bits(raw_system(scene["D"], scene["S"], scene["poses"], stride)[1], out)
    assert same_bits(raw_system(scene["D"], scene["S"], scene["poses"][:1], stride)[1], one)


@pytest.mark.parametrize("kw", [dict(min_weight=3.0), dict(huber=0.1), dict(min_weight=3.0, huber=0.1)])
def test_thresholds_follow_the_restatement(scene, kw):
    base = MR.system(scene["d"], scene["s"], scene["poses"], 1, chunk())
    ref = MR.system(scene["d"], scene["s"], scene["poses"], 1, chunk(), **kw)
    print(kw, "count:", ref[:, 28], "of", base[:, 28])
    if "min_weight" in kw:
        assert (ref[:7, 28] < base[:7, 28]).all() and (ref[:7, 30] < base[:7, 30]).all() and (ref[:7, 28] > 0).all()
    else:
        assert (ref[:, 28] == base[:, 28]).all() and (ref[1:7, 27] < base[1:7, 27]).all()     # the same samples, down-weighted
    rc, out = raw_system(scene["D"], scene["S"], scene["poses"], 1, **kw)
    assert rc == 0 and same_bits(out, ref)


def strided_lattice(target):
    """(dims, stride) of a lattice with sizes in [2, 1024] whose strided lattice has exactly `target` points, or None: a
    factor 1 needs a size of 2 and a stride of 2, a factor a > 1 at stride s the size (a - 1) s + 1."""
    for stride in (1, 2, 3):
        for a in range(1, 1025):
            if target % a:
                continue
            for b in range(a, 1025):
                if (target // a) % b:
                    continue
                c = target // a // b
                if c < b:
                    break
                sizes = [max((f - 1) * stride + 1, 2) for f in (a, b, c)]
                if max(sizes) <= 1024 and all(-(-n // stride) == f for n, f in zip(sizes, (a, b, c))):
                    return tuple(sizes), stride
    return None


def test_chunk_boundaries(scene):
    """Strided lattices of exactly C - 1, C and C + 1 samples where sizes up to 1024 allow it; 2049 = 3 * 683 does not
    (683 is prime), so for C = 2048 the single sample in a chunk of its own is the last of 2 C + 1, with 2 C - 1 and 2 C
    beside it.  S is a synthetic volume (every value unsaturated, every weight 1) laid through D's wall at z = 4."""
    C = chunk()
    assert C in (1024, 2048, 4096)
    targets = [C - 1, C, C + 1 if strided_lattice(C + 1) else None, 2 * C - 1, 2 * C, 2 * C + 1]
    rng = np.random.default_rng(23)
    seen = []
    for target in [t for t in targets if t is not None]:
        found = strided_lattice(target)
        assert found is not None, target
        dims, stride = found
        long_axis = int(np.argmax(dims))
        voxel = 0.9 / (dims[long_axis] - 1)                       # the longest axis spans 0.9 m
        extent = (np.asarray(dims) - 1) * voxel
        # the long axis is turned into D's z by the transform: S's own axes stay lattice axes
        perm = [a for a in range(3) if a != long_axis] + [long_axis]
        R = np.zeros((3, 3))
        for row, a in enumerate(perm):
            R[row, a] = 1.0
        if np.linalg.det(R) < 0:
            R[0] = -R[0]
        centre_d = np.array([0.75, 0.5, 4.0])
        o = centre_d - R @ (0.5 * extent)
        pose = np.concatenate([R, o[:, None]], 1)
        s = MR.volume(rng.uniform(-0.7, 0.7, dims), np.ones(dims), (0.0, 0.0, 0.0), voxel, 0.5)
        S = from_dict(s)
        ref = MR.system(scene["d"], s, pose[None], stride, C)
        print("target", target, "dims", dims, "stride", stride, "count", ref[0, 28], "of", ref[0, 30])
        assert ref[0, 30] == target and ref[0, 28] > 0
        rc, out = raw_system(scene["D"], S, pose[None], stride)
        assert rc == 0 and same_bits(out, ref)
        seen.append(target % C)
    assert {C - 1, 0, 1} <= set(seen)


def test_a_transform_that_leaves_the_destination_is_refused_by_the_step(scene):
    from go_slam_amd import _lib
    rc, rows = raw_system(scene["D"], scene["S"], scene["poses"][6:], 2)
    assert rc == 0 and rows[0, 28] > 64 and rows[1, 28] == 0 and rows[1, 30] > 0 and not rows[1, :28].any()
    rows_d = torch.as_tensor(rows).to(DEV)
    pose_d = torch.as_tensor(scene["poses"][6:].copy()).to(DEV).contiguous()
    trace = torch.full((2, 4), 7.0, dtype=torch.float64, device=DEV)
    rc = _lib.lib().gs_tsdf_align_step(_lib.ptr(rows_d), _lib.ptr(pose_d), 2, 1e-6, 1e-9, 64, _lib.ptr(trace),
                                      _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    ref_pose, ref_trace = AR.step(rows, scene["poses"][6:])
    assert rc == 0 and trace[:, 3].tolist() == [1.0, 0.0]
    assert same_bits(pose_d.cpu().numpy(), ref_pose) and same_bits(trace.cpu().numpy(), ref_trace)
    assert same_bits(pose_d.cpu().numpy()[1], scene["poses"][7])


# ---- a whole registration -------------------------------------------------------------------------------------------
def test_register_equals_the_restatement_and_converges(built_lib):
    """The CPU suite's room: D the three planes off the lattice at 5 cm, S the same room at 4 cm with truncation 0.16 m in
    a frame turned by 12 degrees.  Bit equality hands the CPU suite's convergence assertions to the GPU; they are
    repeated on the GPU's transforms."""
    import test_tsdf_merge_cpu as MC
    tsdf, weight = AR.scene_volume(AR.PLANES_OFF)
    d = MR.volume(tsdf, weight, AR.SCENE_LO, AR.SCENE_VOXEL, AR.SCENE_TRUNC)
    s, _, _ = MC.source(MC.S_FINE)
    D, S = from_dict(d), from_dict(s)
    truth = MC.truth()
    rng = np.random.default_rng(3)
    starts = np.stack([MR.displaced_transform(truth, m, deg, rng) for m, deg in ((0.05, 3.0), (0.10, 5.0), (0.08, 4.0))])
    ref_pose, ref_rows, ref_trace = MR.register(d, s, starts, chunk(), levels=LEVELS)
    res = D.register(S, starts, levels=LEVELS)
    assert same_bits(res["T"][:, :3, :], ref_pose) and np.array_equal(res["T"][:, 3], np.tile([0, 0, 0, 1.0], (3, 1)))
    assert same_bits(res["trace"], ref_trace) and res["trace"].shape == (20, 3, 4)
    assert res["ok"].all() and (res["count"] == ref_rows[:, 28]).all()
    assert same_bits(res["rmse_m"], AR.SCENE_TRUNC * np.sqrt(ref_rows[:, 29] / ref_rows[:, 28]))
    assert same_bits(res["overlap"], ref_rows[:, 28] / ref_rows[:, 30]) and (res["overlap"] == 1.0).all()
    errs = np.array([AR.pose_error(p[:3], truth) for p in res["T"]])
    pairs = np.array([AR.pose_error(p[:3], q[:3]) for i, p in enumerate(res["T"]) for q in res["T"][i + 1:]])
    print("errors against the truth (m, deg):", errs.tolist(), "moved:", res["moved_m"], res["moved_deg"], "rmse", res["rmse_m"])
    MC.assert_converged(s, ref_rows, res["trace"], errs, pairs, d)
    assert (res["n_constrained"] == 3).all() and np.abs(res["moved_constrained_m"] - res["moved_m"]).max() <= 1e-15
    again = D.register(S, starts, levels=LEVELS)
    assert same_bits(again["T"], res["T"]) and same_bits(again["trace"], res["trace"])
    one = D.register(S, starts[1], levels=LEVELS)                                    # one [3,4] transform
    assert same_bits(one["T"][0], res["T"][1])


# ---- the merge --------------------------------------------------------------------------------------------------------
def raw_merge(dst, src, d2s, min_weight=1.0, colors=True, max_weight=None):
    from go_slam_amd import _lib
    m = np.ascontiguousarray(d2s, np.float32)
    rc = _lib.lib().gs_tsdf_merge(_lib.ptr(dst.tsdf), _lib.ptr(dst.weight), _lib.ptr(dst.colors) if colors else None,
                                  *lattice_args(dst), dst.max_weight if max_weight is None else max_weight,
                                  _lib.ptr(src.tsdf), _lib.ptr(src.weight), _lib.ptr(src.colors) if colors else None,
                                  *lattice_args(src), m.ctypes.data_as(ctypes.c_void_p), min_weight, _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("empty", [False, True])
@pytest.mark.parametrize("min_weight", [1.0, 3.0])
def test_merge_equals_the_restatement_bit_for_bit(scene, empty, min_weight):
    """S (truncation 0.625 m) into D (0.5 m): ratio 1.25, so s < -1 skips and fminf(1, s) holds.  Into the fused D and into
    an empty one; tsdf, weight and colours bit for bit, every skipped point with the bits it had."""
    D = TG.volume() if empty else copy_of(scene["D"])
    before = as_dict(D)
    ref = MR.merge(before, scene["s"], MR.inverse(scene["T"]), min_weight=min_weight)
    touched = ref["touched"]
    print("touched", touched.sum(), "of", touched.size, "; clamped to 1:", (ref["tsdf"][touched] == 1).sum())
    assert 0.05 < touched.mean() < 0.9
    D._flags = "stale"
    assert D.merge(scene["S"], four(scene["T"]), min_weight=min_weight) is D and D._flags is None
    assert same_state(D, ref)
    for name in ("tsdf", "weight"):
        assert np.array_equal(TG.bits(getattr(D, name))[~touched], TG.bits(before[name])[~touched])
    assert np.array_equal(TG.bits(D.colors)[:, ~touched], TG.bits(before["colors"])[:, ~touched])
    assert (TG.bits(D.weight)[touched] != TG.bits(before["weight"])[touched]).all()


def test_merge_without_colours_leaves_them_alone(scene):
    for empty in (False, True):
        D = TG.volume() if empty else copy_of(scene["D"])
        before = as_dict(D)
        ref = MR.merge({k: v for k, v in before.items() if k != "colors"}, scene["s"], MR.inverse(scene["T"]))
        assert raw_merge(D, scene["S"], MR.inverse(scene["T"]), colors=False) == 0
        assert same_state(D, ref, colors=False) and np.array_equal(TG.bits(D.colors), TG.bits(before["colors"]))
        full = MR.merge(before, scene["s"], MR.inverse(scene["T"]))
        assert np.array_equal(TG.bits(full["tsdf"]), TG.bits(ref["tsdf"]))         # colours change nothing else


def test_a_source_outside_the_destination_changes_nothing(scene):
    D = copy_of(scene["D"])
    before = as_dict(D)
    far = scene["T"].copy()
    far[:, 3] += [40.0, 0.0, 0.0]
    assert not MR.merge(before, scene["s"], MR.inverse(far))["touched"].any()
    D.merge(scene["S"], far)
    assert same_state(D, before)
    near = scene["T"].copy()                                    # S's box ends inside D's first tiles: a tile test that skipped
    near[:, 3] += [-4.0, 0.0, 0.0]                              # too eagerly would show here
    ref = MR.merge(before, scene["s"], MR.inverse(near))
    print("touched with S moved by -4 m along x:", ref["touched"].sum())
    assert 0 < ref["touched"].sum() < 0.2 * ref["touched"].size
    D.merge(scene["S"], near)
    assert same_state(D, ref)


def test_two_merges_reach_the_weight_cap(scene):
    D = TG.volume(max_weight=4.0)
    ref = MR.merge(MR.merge(as_dict(D), scene["s"], MR.inverse(scene["T"]), max_weight=4.0), scene["s"],
                   MR.inverse(scene["T"]), max_weight=4.0)
    t = ref["touched"]
    assert ref["weight"].max() == 4.0 and (ref["weight"][t] == 4.0).sum() > 1000 and (ref["weight"][t] < 4.0).sum() > 100
    D.merge(scene["S"], scene["T"]).merge(scene["S"], scene["T"])
    assert same_state(D, ref)


def test_join_volumes_registers_and_merges(scene):
    """Both fused volumes into a union volume in D's world, from a start 2 cm / 1 degree off: the union encloses both
    boxes, the registered transform ends nearer the truth than it began, and the joined lattice is the restatement's
    merge of the two at the transforms `join_volumes` returned."""
    from go_slam_amd import tsdf_merge as TM
    start = scene["poses"][1]
    joined, transforms, reports = TM.join_volumes([scene["D"], scene["S"]], [None, four(start)], levels=LEVELS)
    assert np.array_equal(transforms[0], np.eye(4)) and reports[0] == {"registered": False, "ok": True}
    rep = reports[1]
    e0, e1 = AR.pose_error(start, scene["T"]), AR.pose_error(transforms[1][:3], scene["T"])
    print("start", e0, "end", e1, "report", {k: v for k, v in rep.items() if k != "T"})
    assert rep["ok"] and rep["registered"] and 0 < rep["overlap"] < 1 and rep["count"] > 1000
    assert joined.voxel == TG.VOXEL and joined.trunc == 0.5 and e1[1] < e0[1]
    hi = joined.lo + (np.asarray(joined.dims) - 1) * joined.voxel
    for vol, T in ((scene["D"], np.eye(4)), (scene["S"], transforms[1])):
        box = TM.moved_box(vol, T[:3])
        assert (box >= joined.lo - 1e-9).all() and (box <= hi + 1e-9).all()
    ref = MR.empty_volume(joined.dims, joined.lo, joined.voxel, joined.trunc)
    ref = MR.merge(ref, scene["d"], None)
    ref = MR.merge(ref, scene["s"], MR.inverse(transforms[1][:3]))
    assert same_state(joined, ref)
    with pytest.raises(ValueError, match="registration of volume 1 failed"):
        TM.join_volumes([scene["D"], scene["S"]], [None, four(scene["poses"][7])], levels=LEVELS)
    given, transforms, reports = TM.join_volumes([scene["D"], scene["S"]], [None, four(scene["T"])], register=False)
    assert same_bits(transforms[1][:3], scene["T"]) and reports[1] == {"registered": False, "ok": True}


# ---- the C ABI's refusals -----------------------------------------------------------------------------------------------
def guarded(n, fill, dtype=torch.float32):
    buf = torch.full((2 * GUARD + n,), fill, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def test_bad_arguments_are_refused_without_a_write(scene):
    """Every refusal of the C ABI returns GS_ERR_INVALID_ARG (-1) before a launch: the rows, the workspace and the
    destination's lattices, each between guard bands, keep their fill."""
    from go_slam_amd import _lib
    L = _lib.lib()
    D, S = scene["D"], scene["S"]
    fill = 7.0
    n_ws = L.gs_tsdf_register_workspace_bytes(2, *S.dims, 1) // 8
    out_buf, out = guarded(64, fill, torch.float64)
    ws_buf, ws = guarded(n_ws, fill, torch.float64)
    pose = torch.as_tensor(scene["poses"][:2].copy()).to(DEV).contiguous()
    names = ("nx", "ny", "nz", "lox", "loy", "loz", "voxel", "trunc")
    good = dict(tsdf_d=D.tsdf, weight_d=D.weight, **{f"{k}_d": v for k, v in zip(names, lattice_args(D))}, tsdf_s=S.tsdf,
                weight_s=S.weight, **{f"{k}_s": v for k, v in zip(names, lattice_args(S))}, pose=pose, B=2, stride=1,
                min_weight=1.0, huber=0.5, ws=ws, out=out)
    order = ["tsdf_d", "weight_d"] + [f"{k}_d" for k in names] + ["tsdf_s", "weight_s"] + [f"{k}_s" for k in names] + \
        ["pose", "B", "stride", "min_weight", "huber", "ws", "out"]

    def call(**bad):
        a = dict(good, **bad)
        return L.gs_tsdf_register_system(*[(_lib.ptr(a[k]) if isinstance(a[k], torch.Tensor) or a[k] is None else a[k])
                                           for k in order], _lib.stream_ptr(DEV))

    bads = [dict(nx_d=1), dict(ny_d=1025), dict(nz_d=0), dict(nx_s=1), dict(ny_s=1025), dict(nz_s=-3), dict(B=-1),
            dict(stride=0), dict(stride=-2), dict(voxel_d=0.0), dict(voxel_d=math.inf), dict(voxel_s=-0.1),
            dict(voxel_s=math.nan), dict(trunc_d=0.0), dict(trunc_d=math.nan), dict(trunc_s=-0.5), dict(trunc_s=math.inf),
            dict(lox_d=math.nan), dict(loz_s=math.inf), dict(huber=0.0), dict(huber=-1.0), dict(huber=math.nan),
            dict(min_weight=math.nan), dict(tsdf_d=None), dict(weight_d=None), dict(tsdf_s=None), dict(weight_s=None),
            dict(pose=None), dict(ws=None), dict(out=None)]
    for bad in bads:
        assert call(**bad) == -1, bad
        assert L.gs_last_error().startswith(b"tsdf_register_system"), bad
    assert call(B=0) == 0                                       # nothing to do, nothing launched
    torch.cuda.synchronize()
    assert bool((out_buf == fill).all()) and bool((ws_buf == fill).all())
    assert L.gs_tsdf_register_workspace_bytes(-1, *S.dims, 1) == 0 and L.gs_tsdf_register_workspace_bytes(2, *S.dims, 0) == 0
    assert call() == 0                                          # and the good call does write
    torch.cuda.synchronize()
    assert bool((out != fill).any()) and bool((out_buf[:GUARD] == fill).all()) and bool((out_buf[-GUARD:] == fill).all())

    # gs_tsdf_merge: a small destination whose every element would change if anything ran (weights 7 >= min_weight)
    dims_d, dims_s = (5, 4, 6), (6, 5, 7)
    nd = 5 * 4 * 6
    t_buf, t = guarded(nd, fill)
    w_buf, w = guarded(nd, fill)
    c_buf, c = guarded(3 * nd, fill)
    src = [torch.full(dims_s, 0.5, device=DEV), torch.full(dims_s, 2.0, device=DEV), torch.full((3,) + dims_s, 0.5, device=DEV)]
    eye = np.concatenate([np.eye(3), np.zeros((3, 1))], 1).astype(np.float32)
    mnames = ("nx", "ny", "nz", "lox", "loy", "loz", "voxel", "trunc")
    mgood = dict(tsdf_d=t, weight_d=w, colors_d=c, **dict(zip([f"{k}_d" for k in mnames], [*dims_d, 0.0, 0.0, 0.0, 0.1, 0.4])),
                 max_weight=64.0, tsdf_s=src[0], weight_s=src[1], colors_s=src[2],
                 **dict(zip([f"{k}_s" for k in mnames], [*dims_s, -0.05, -0.05, -0.05, 0.1, 0.5])), d2s=eye, min_weight=1.0)
    morder = ["tsdf_d", "weight_d", "colors_d"] + [f"{k}_d" for k in mnames] + ["max_weight", "tsdf_s", "weight_s", "colors_s"] + \
        [f"{k}_s" for k in mnames] + ["d2s", "min_weight"]

    def arg(v):
        if isinstance(v, torch.Tensor) or v is None:
            return _lib.ptr(v)
        return v.ctypes.data_as(ctypes.c_void_p) if isinstance(v, np.ndarray) else v

    def merge(**bad):
        a = dict(mgood, **bad)
        rc = L.gs_tsdf_merge(*[arg(a[k]) for k in morder], _lib.stream_ptr(DEV))
        torch.cuda.synchronize()
        return rc

    nan_eye, inf_eye = eye.copy(), eye.copy()
    nan_eye[1, 1], inf_eye[2, 3] = math.nan, math.inf
    mbads = [dict(nx_d=1), dict(nz_d=1025), dict(ny_s=0), dict(nx_s=2000), dict(voxel_d=0.0), dict(voxel_s=math.nan),
             dict(voxel_s=math.inf), dict(trunc_d=0.0), dict(trunc_s=math.nan), dict(trunc_s=0.39), dict(trunc_d=0.51),
             dict(lox_d=math.nan), dict(loy_s=math.inf), dict(max_weight=0.5), dict(max_weight=math.nan), dict(min_weight=0.0),
             dict(min_weight=-1.0), dict(min_weight=math.nan), dict(tsdf_d=None), dict(weight_d=None), dict(tsdf_s=None),
             dict(weight_s=None), dict(d2s=None), dict(d2s=nan_eye), dict(d2s=inf_eye),
             dict(tsdf_s=t, weight_s=w, colors_s=c, nx_s=5, ny_s=4, nz_s=6)]
    for bad in mbads:
        assert merge(**bad) == -1, bad
        assert L.gs_last_error().startswith(b"tsdf_merge"), bad
    for buf in (t_buf, w_buf, c_buf):
        assert bool((buf == fill).all())
    assert merge(colors_d=None) == 0                            # colours on one side only: fused without them
    assert bool((c_buf == fill).all()) and bool((t[:-1] != fill).any()) and bool((t_buf[:GUARD] == fill).all())
    assert bool((t_buf[-GUARD:] == fill).all()) and bool((w_buf[:GUARD] == fill).all()) and bool((w_buf[-GUARD:] == fill).all())


# ---- a second run joined with the first ---------------------------------------------------------------------------------
def test_second_run_is_joined_with_the_first_runs_volume(built_lib, tmp_path, monkeypatch):
    """Two sessions that each map a part of the site: a first 16-frame only-tracking rgbd run fuses x <= 1 m and saves
    its volume; a second run of the same frames fuses x >= -1 m, says its world is 2 cm off along y and z (the wall's and
    the floor's normals), registers that away over the two metres both saw and joins the two.  (The same bound in both runs
    would show the merge's rim instead: a point of the destination takes a value only from a source cell seen at all
    eight corners, so the outermost seen layer of a volume does not reach the joined one -- 2609 faces against 2778 of
    either run's own mesh when both runs fuse the whole scene.)"""
    from go_slam_amd import tsdf_merge as TM
    from go_slam_amd.neus.mesh import load_mesh
    from go_slam_amd.slam import SLAM
    from go_slam_amd.tsdf import TSDFVolume
    returned = []
    terminate = SLAM.terminate

    def keeping(self, *args, **kw):
        returned.append(terminate(self, *args, **kw))
        return returned[-1]
    monkeypatch.setattr(SLAM, "terminate", keeping)
    first, second = str(tmp_path / "first"), str(tmp_path / "second")
    base = {"enable": True, "source": "sensor", "voxel_size": 0.1, "save_volume": True}
    TG.whole_run(first, dict(base, bound=[[-4.0, 1.0], [-3.0, 2.0], [-1.0, 5.0]]))
    init = np.eye(4)
    init[1:3, 3] = [0.02, -0.02]
    TG.whole_run(second, dict(base, bound=[[-1.0, 4.0], [-3.0, 2.0], [-1.0, 5.0]],
                              merge={"enable": True, "volume": f"{first}/mesh/tsdf_volume.npz", "init": init.tolist(),
                                           "levels": [[2, 10], [1, 10]], "save_volume": True}))
    text = open(f"{second}/metrics_tsdf_merge.txt").read()
    print(text)
    result, T = TM.parse_merge(text)
    assert TM.merge_text(result, T) == text                     # the text round trip, bit for bit
    stats = returned[1]
    assert stats["tsdf_merge_overlap"] == result["overlap"] and stats["tsdf_merge_rmse_m"] == result["rmse_m"]
    assert stats["tsdf_merge_moved_m"] == result["moved_m"] and stats["tsdf_merge_ok"] is True and result["ok"] == 1
    assert set(returned[1]) - set(returned[0]) == {"tsdf_merge_overlap", "tsdf_merge_rmse_m", "tsdf_merge_moved_m",
                                                   "tsdf_merge_ok"}
    assert result["registered"] == 1 and result["overlap"] > 0.25 and result["count"] >= 64
    # both runs fused the same frames at the same poses: the true transform is the identity, and the start was 2.8 cm off
    # along the two directions the wall and the floor hold
    print("left of the 2 cm offsets:", T[1:3, 3], "rotation", AR.pose_error(T, np.eye(4)[:3])[1], "deg")
    assert np.abs(T[1:3, 3]).max() < 0.005
    own = [len(load_mesh(f"{d}/mesh/tsdf_mesh.ply").faces) for d in (first, second)]
    merged = len(load_mesh(f"{second}/mesh/tsdf_merged_mesh.ply").faces)
    print("faces:", own, "merged:", merged)
    assert merged >= max(own)
    vol = TSDFVolume.load(f"{second}/mesh/tsdf_merged_volume.npz", device=DEV)
    one = TSDFVolume.load(f"{first}/mesh/tsdf_volume.npz", device=DEV)
    assert vol.voxel == one.voxel and vol.trunc == one.trunc and vol.dims[0] > one.dims[0]
    assert all(a <= b <= a + 1 for a, b in zip(one.dims[1:], vol.dims[1:]))        # the moved box is a hair off the lattice
    assert float(vol.weight.max()) >= float(one.weight.max()) and float(vol.tsdf.min()) < 0
    assert min(own) > 500                                       # each session saw a good part of the scene
    new = {"metrics_tsdf_merge.txt", os.path.join("mesh", "tsdf_merged_mesh.ply"), os.path.join("mesh", "tsdf_merged_volume.npz")}
    assert [p for p in TG.listing(second) if p not in new] == TG.listing(first)
    assert new <= set(TG.listing(second))
