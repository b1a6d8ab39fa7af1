"""The TSDF fusion kernels on the MI355X against truth that is not their restatement.

1. gs_tsdf_integrate and gs_tsdf_accumulate + gs_tsdf_resolve on turned_scene() (tests/tsdf_fusion_scene.py: twenty
   turned and rolled cameras, fx != fy, an asymmetric principal point, a painted room) against tests/tsdf_fusion_model.py, per
   clean lattice point and under the model's own bounds: tests/test_tsdf_fusion_model_cpu.py's comparison, unchanged.
   Nothing computed on the GPU acts as referee.
2. The painted room end to end: integrate -> raycast, accumulate -> resolve -> raycast, and two volumes on different
   lattices merged -> raycast, from three views that were not fused, and extract_mesh; depth against the analytic
   depth, colour against the paint at the analytic hit.
3. The frustum skip of the shared sweep against the restatements, which have none, bit for bit, on small lattices and
   cameras chosen to sit where a skip could go wrong.

MEASURED (MI355X).  None of the GPU figures is a tolerance: the bounds of 1 are the model's own, those of 2 are the CPU
figures times 1.1, and 3 is bit for bit.
  1. worst error / bound over the grid (the error and the bound at that element), clean points only
     gs_tsdf_integrate                    tsdf 0.290 (7.340e-07 / 2.529e-06)   colour 0.438 (7.6e-09 / 1.7e-08)
     gs_tsdf_accumulate + gs_tsdf_resolve tsdf 0.958 (3.032e-05 / 3.164e-05)   colour 1.000 (1.961e-03 / 1.961e-03)
     weights, counts and count_rgb exact; unobserved clean points fresh.  A point seen once meets the half quantum of
     its colour; the CPU restatements give the same figures.  Excluded: 0.086 % (masked) and 0.070 % of the observed
     pairs undecided, 0.14 % of the points not clean, 39.8 % and 41.6 % of the lattice observed.
  2. worst error at a hit            depth, float64 restatements | GPU     colour, float64 restatements | GPU     hits
     integrate -> raycast             0.100834974 | 0.100835097 m      0.050305893 | 0.050305848       661 565 479
     accumulate -> resolve -> raycast 0.100834750 | 0.100834859 m      0.050464740 | 0.050464694       661 565 479
     merge of two lattices -> raycast 0.099351063 | 0.099351031 m      0.041905172 | 0.041905242       644 520 453
     extract_mesh(3.0): 993 vertices, worst distance 0.045218 m, worst colour 0.026728 (the float64 mesh: the same)
  3. share of the (z-run, frame) pairs without an observed point / with observed and unobserved points
     3 x 6 x 2     voxel 0.11                          0.698 / 0.176
     4 x 3 x 63    voxel 0.11                          0.425 / 0.575
     6 x 4 x 64    voxel 0.11                          0.464 / 0.535
     5 x 5 x 65    voxel 0.11                          0.726 / 0.257
     3 x 4 x 130   voxel 0.11                          0.766 / 0.226
     5 x 5 x 65    voxel 0.11, lo (512.3, -300.7, 801.1) 0.704 / 0.269
     4 x 5 x 65    voxel 0.05                          0.704 / 0.273
     4 x 3 x 64    voxel 0.7                           0.436 / 0.564
     every state of both kernels equal to its restatement bit for bit, under each of the four intrinsics.
No kernel, restatement or header text was found wrong.
"""
import math

import numpy as np
import pytest
import torch

import tsdf_fusion_scene as S
import tsdf_live_restatement as LR
import tsdf_restatement as TR
import test_tsdf_fusion_model_cpu as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SC = C.SC


@pytest.fixture(autouse=True)
def _stop_after_a_device_error():
    """a failed assertion lets the next test run; a device error ends the session (nothing more is launched after it)"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as exc:
        pytest.exit(f"device error, stopping: {exc}", returncode=3)


def tensors(sel=slice(None), images=True, mask=True):
    """integrate's / accumulate's arguments for the frames `sel` of the scene"""
    return ((torch.from_numpy(SC["depth"][sel]), torch.from_numpy(SC["w2c"][sel]), S.INTR),
            {"images": torch.from_numpy(SC["images"][sel]) if images else None,
             "mask": torch.from_numpy(SC["mask"][sel]) if mask else None})


def volume(lo=S.LO, dims=S.DIMS, voxel=S.VOXEL, max_weight=64.0):
    from go_slam_amd.tsdf import TSDFVolume
    vol = TSDFVolume(S.bound_of(lo, dims, voxel), voxel, trunc=S.TRUNC, max_weight=max_weight, device=DEV)
    assert vol.dims == tuple(dims) and np.array_equal(vol.lo, np.asarray(lo, np.float64))
    return vol


def reversible():
    from go_slam_amd.tsdf_live import ReversibleTSDF
    vol = ReversibleTSDF(S.bound_of(S.LO, S.DIMS, S.VOXEL), S.VOXEL, trunc=S.TRUNC, device=DEV)
    assert vol.dims == S.DIMS
    return vol


def host(vol):
    return {k: getattr(vol, k).cpu().numpy() for k in ("tsdf", "weight", "colors")}


# ---- 1. the kernels against the model --------------------------------------------------------------------------------
@pytest.mark.parametrize("max_weight,images,mask", C.GRID)
def test_integrate_against_the_model_per_element(built_lib, max_weight, images, mask):
    args, kw = tensors(images=images, mask=mask)
    vol = volume(max_weight=max_weight).integrate(*args, **kw)
    C.check_integrate(host(vol), max_weight, images, mask, "gs_tsdf_integrate")


@pytest.mark.parametrize("images", [True, False])
@pytest.mark.parametrize("mask", [True, False])
def test_accumulate_and_resolve_against_the_model_per_element(built_lib, images, mask):
    """All frames added, then a third of them taken out with sign -1."""
    alive = np.arange(len(SC["depth"])) % 3 != 1
    out = np.nonzero(~alive)[0]
    rev = reversible()
    args, kw = tensors(images=images, mask=mask)
    rev.accumulate(*args, **kw)
    args, kw = tensors(out, images=images, mask=mask)
    rev.accumulate(*args, sign=-1, **kw)
    assert rev.n_live == int(alive.sum())
    C.check_resolved(host(rev.resolve()), rev.count_rgb.cpu().numpy(), alive, images, mask,
                     "gs_tsdf_accumulate + gs_tsdf_resolve")


def test_the_caps_hold_on_the_scene_the_kernels_are_judged_on():
    C.test_caps_on_what_the_model_leaves_undecided()


# ---- 2. the painted room, end to end ---------------------------------------------------------------------------------
# Worst |depth - analytic depth| (metres) and worst |colour - paint at the analytic hit| over the hits of the three views,
# measured on the CPU with the float64 forms of the restatements (tsdf_fusion_scene.reference_pipelines(np.float64):
# tsdf_restatement.integrate, tsdf_merge_restatement.merge and tsdf_raycast_restatement.raycast with dtype=np.float64;
# tsdf_live_restatement's integer state has no float64 form, its resolved volume is raycast in float64), not on the
# kernels.  `python tests/tsdf_fusion_scene.py` prints them, and tests/test_tsdf_fusion_model_cpu.py recomputes them and
# checks what makes them usable: each depth figure below one voxel, each colour figure below the paint's Lipschitz
# constant times two voxels, at least half of every view's pixels hit.
DEPTH_FP64_MAX = {"integrate": 0.10083497432833388, "reversible": 0.1008347501304443, "merge": 0.09935106348718836}
COLOUR_FP64_MAX = {"integrate": 0.050305893040317406, "reversible": 0.050464740042619805, "merge": 0.04190517243826686}
MESH_MIN_WEIGHT = 3.0       # see test_the_painted_room_as_a_mesh


def view_pipeline(name):
    from go_slam_amd.tsdf_merge import merge_volume
    if name == "integrate":
        args, kw = tensors()
        return volume().integrate(*args, **kw)
    if name == "reversible":
        args, kw = tensors()
        return reversible().accumulate(*args, **kw).resolve()
    args, kw = tensors(slice(0, None, 2))
    src = volume().integrate(*args, **kw)
    args, kw = tensors(slice(1, None, 2))
    dst = volume(S.LO_D, S.DIMS_D, S.VOXEL_D).integrate(*args, **kw)
    return merge_volume(dst, src, np.concatenate([np.eye(3), np.zeros((3, 1))], 1))


@pytest.mark.parametrize("name", ["integrate", "reversible", "merge"])
def test_the_painted_room_through_fusion_and_raycast(built_lib, name):
    """At every hit of three views that were not fused (24 x 32, one rolled): the depth against the analytic depth and
    the colour against the paint at the analytic hit point, each held to the float64 restatements' own worst error plus
    10 %, the project's margin for "fp32 against fp64 only moves values by roundings"."""
    assert DEPTH_FP64_MAX[name] < (S.VOXEL_D if name == "merge" else S.VOXEL), "the scene is wrong, not the kernel"
    assert COLOUR_FP64_MAX[name] < S.PAINT_LIPSCHITZ * 2 * (S.VOXEL_D if name == "merge" else S.VOXEL)
    vol = view_pipeline(name)
    cast = vol.raycast(torch.from_numpy(S.w2c32(S.VIEWS)), S.VIEW_INTR, S.VIEW_SIZE)
    depth, colour, hits = S.view_errors({k: cast[k].cpu().numpy() for k in ("depth", "color")})
    print(f"{name}: hits per view {hits.tolist()} of {S.VIEW_SIZE[0] * S.VIEW_SIZE[1]}; worst depth error {depth:.9f} m "
          f"(float64 restatements {DEPTH_FP64_MAX[name]:.9f}), worst colour error {colour:.9f} "
          f"(float64 restatements {COLOUR_FP64_MAX[name]:.9f})")
    assert (hits >= S.VIEW_SIZE[0] * S.VIEW_SIZE[1] // 2).all()
    assert depth <= 1.1 * DEPTH_FP64_MAX[name]
    assert colour <= 1.1 * COLOUR_FP64_MAX[name]


def test_the_painted_room_as_a_mesh(built_lib):
    """extract_mesh on the integrated volume: every kept vertex within the integrate pipeline's depth figure of its
    nearest surface, its colour within the colour figure (plus 1 / 255 for the u8 rounding) of the paint there.  Kept
    means between lattice points seen three times: at the lattice's border x = lo.x the floor is seen once or twice, by
    cameras that graze it, a vertex there carries one pixel's colour from 0.15 m away, and the float64 restatement's
    own mesh is 0.114 off the paint there (0.027 with three observations, 0.018 at the 99th percentile either way).  The
    raycast views do not look at that border; the figures are theirs."""
    args, kw = tensors()
    mesh = volume().integrate(*args, **kw).extract_mesh(MESH_MIN_WEIGHT)
    dist, colour = S.mesh_errors(mesh.vertices, mesh.vertex_colors)
    print(f"{len(mesh.vertices)} vertices: worst distance {dist:.6f} m, worst colour error {colour:.6f}")
    assert len(mesh.faces) > 1000 and len(mesh.vertices) > 800
    assert dist <= 1.1 * DEPTH_FP64_MAX["integrate"]
    assert colour <= 1.1 * COLOUR_FP64_MAX["integrate"] + 1.0 / 255.0


# ---- 3. the frustum skip cannot change a result ----------------------------------------------------------------------
SKIP_HW = (20, 28)
SKIP_INTRINSICS = {"plain": (19.0, 17.5, 13.25, 10.75), "principal point outside": (19.0, 17.5, -5.0, SKIP_HW[0] + 5.0),
                   "narrower than a voxel": (2000.0, 2000.0, 13.25, 10.75), "wider than 140 degrees": (4.0, 4.0, 13.25, 10.75)}
SKIP_KINDS = ("inside", "along +z", "along -z", "side plane across the run", "roll 90", "roll 45", "sees nothing",
              "side plane across the run")
SKIP_CAMERAS = 48
# (dims, voxel, lo)
SKIP_LATTICES = [((3, 6, 2), 0.11, (-0.17, -0.29, 0.13)), ((4, 3, 63), 0.11, (-0.17, -0.29, 0.13)),
                 ((6, 4, 64), 0.11, (-0.17, -0.29, 0.13)), ((5, 5, 65), 0.11, (-0.17, -0.29, 0.13)),
                 ((3, 4, 130), 0.11, (-0.17, -0.29, 0.13)), ((5, 5, 65), 0.11, (512.3, -300.7, 801.1)),
                 ((4, 5, 65), 0.05, (-0.17, -0.29, 0.13)), ((4, 3, 64), 0.7, (-0.17, -0.29, 0.13))]


def frame_of(forward, roll_deg):
    """camera-to-world rotation with the optical axis `forward` (unit), rolled about it; exact 0 and +-1 entries for an
    axis along +-z without roll"""
    f = np.asarray(forward, np.float64)
    if abs(f[2]) == 1.0:
        right, down = np.array([f[2], 0.0, 0.0]), np.array([0.0, 1.0, 0.0])
    else:
        right = np.cross([0.0, 1.0, 0.0], f) if abs(f[1]) < 0.9 else np.cross(f, [0.0, 0.0, 1.0])
        right /= np.linalg.norm(right)
        down = np.cross(f, right)
    R = np.stack([right, down, f], 1)
    if roll_deg:
        c, s = math.cos(math.radians(roll_deg)), math.sin(math.radians(roll_deg))
        R = R @ np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    return R


def skip_frames(dims, voxel, lo, intr, seed):
    """SKIP_CAMERAS frames about the lattice, the kinds in turn: (depth, w2c, images, mask) as float32.  A camera is
    turned as its kind says and then placed so that the ray through the middle of its image (which is far from the
    optical axis when the principal point lies outside) passes through a lattice point T, from a few to a few dozen
    voxels away, or, for the kind that sees nothing, so that T lies as far behind it.  Its depth image is T's depth along
    the optical axis less one truncation, plus two voxels of per-pixel noise: the far limit sdf >= -trunc of what the
    frame observes then passes through the lattice near T and cuts runs."""
    g = np.random.default_rng(seed)
    h, w = SKIP_HW
    fx, fy, cx, cy = intr
    lo = np.asarray(lo, np.float64)
    middle = np.array([(0.5 * (w - 1) - cx) / fx, (0.5 * (h - 1) - cy) / fy, 1.0])
    middle /= np.linalg.norm(middle)
    depth, mats = [], []
    for n in range(SKIP_CAMERAS):
        kind = SKIP_KINDS[n % len(SKIP_KINDS)]
        T = lo + g.integers(0, dims) * voxel
        far = voxel * g.uniform(3.0, 30.0)
        rnd = g.normal(size=3)
        rnd /= np.linalg.norm(rnd)
        roll = {"roll 90": 90.0, "roll 45": 45.0}.get(kind, 0.0)
        if kind in ("along +z", "along -z"):
            fwd = np.array([0.0, 0.0, 1.0 if kind == "along +z" else -1.0])
        elif kind == "side plane across the run":
            a = g.uniform(0, 2 * math.pi)
            fwd = np.array([math.cos(a), math.sin(a), 0.0])
        else:
            fwd = rnd
        R = frame_of(fwd, roll)
        if kind == "inside":
            q = lo + g.random(3) * (np.asarray(dims) - 1) * voxel
        else:
            q = T - (-far if kind == "sees nothing" else far) * (R @ middle)
        mats.append(np.concatenate([R.T, -(R.T @ q)[:, None]], 1))
        surface = max(float(fwd @ (T - q)) - 4 * voxel, voxel)
        depth.append(surface + voxel * g.uniform(-2.0, 2.0, (h, w)))
    K = SKIP_CAMERAS
    return (np.stack(depth).astype(np.float32), np.stack(mats).astype(np.float32), g.random((K, 3, h, w), dtype=np.float32),
            (g.random((K, h, w)) > 0.2).astype(np.float32))


def run_shares(dims, voxel, lo, intr, frames):
    """(pairs, pairs with no observed point, pairs with observed and unobserved points) over the (z-run, frame) pairs,
    from the restatement's own per-frame selection"""
    depth, mats, _, mask = frames
    nx, ny, nz = dims
    chunks = -(-nz // 64)
    px, py, pz = TR.lattice_axes(dims, lo, voxel)
    size = np.minimum(64, nz - 64 * np.arange(chunks))
    none = mixed = 0
    for f in range(len(depth)):
        sel, _, _, _ = TR.frame_geometry(f, depth, mats, intr, px, py, pz, 4 * voxel, mask)
        seen = np.zeros(nx * ny * nz, bool)
        seen[sel] = True
        per_run = np.add.reduceat(seen.reshape(nx * ny, nz), 64 * np.arange(chunks), axis=1)
        none += int((per_run == 0).sum())
        mixed += int(((per_run > 0) & (per_run < size[None, :])).sum())
    return len(depth) * nx * ny * chunks, none, mixed


def bits(t):
    t = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t
    return np.ascontiguousarray(t, dtype=np.float32).view(np.int32)


@pytest.mark.parametrize("case", range(len(SKIP_LATTICES)), ids=lambda n: "x".join(map(str, SKIP_LATTICES[n][0])) +
                         f"-voxel{SKIP_LATTICES[n][1]}-lo{SKIP_LATTICES[n][2][0]}")
def test_the_frustum_skip_cannot_change_a_result(built_lib, case):
    """gs_tsdf_integrate (coloured) and gs_tsdf_accumulate against their restatements, bit for bit, for 48 cameras (three
    batches) under each of four intrinsics.  Two conditions, from the restatement's selections: at least 30 % of the
    (z-run, frame) pairs have no observed point (there is something to skip) and at least 10 % have both kinds (the
    skip's boundary is exercised)."""
    from go_slam_amd.tsdf import TSDFVolume
    from go_slam_amd.tsdf_live import ReversibleTSDF
    dims, voxel, lo = SKIP_LATTICES[case]
    bound = S.bound_of(lo, dims, voxel)
    total = none = mixed = 0
    for n, (name, intr) in enumerate(SKIP_INTRINSICS.items()):
        frames = skip_frames(dims, voxel, lo, intr, seed=100 * case + n)
        depth, mats, images, mask = frames
        t, a, b = run_shares(dims, voxel, lo, intr, frames)
        total, none, mixed = total + t, none + a, mixed + b
        ref = TR.integrate(TR.new_volume(dims), depth, mats, intr, lo, voxel, 4 * voxel, 64.0, images=images, mask=mask)
        state = LR.accumulate(LR.new_state(dims), depth, mats, intr, lo, voxel, 4 * voxel, images=images, mask=mask)
        vol = TSDFVolume(bound, voxel, device=DEV)
        rev = ReversibleTSDF(bound, voxel, device=DEV)
        assert vol.dims == tuple(dims) and rev.dims == tuple(dims) and np.float32(vol.trunc) == np.float32(4 * voxel)
        args = (torch.from_numpy(depth), torch.from_numpy(mats), intr)
        kw = {"images": torch.from_numpy(images), "mask": torch.from_numpy(mask)}
        vol.integrate(*args, **kw)
        rev.accumulate(*args, **kw)
        for k in ("tsdf", "weight", "colors"):
            assert np.array_equal(bits(getattr(vol, k)), bits(ref[k])), (name, k)
        for k, got in zip(("sum_s", "count", "sum_rgb", "count_rgb"), rev.state()):
            assert np.array_equal(got.cpu().numpy(), state[k]), (name, k)
        print(f"  {name}: {a / t:.3f} of the pairs without an observed point, {b / t:.3f} with both kinds, "
              f"{(ref['weight'] > 0).mean():.3f} of the points observed")
    print(f"lattice {dims} voxel {voxel} lo {lo}: {none / total:.3f} without an observed point, {mixed / total:.3f} with both")
    assert none >= 0.30 * total and mixed >= 0.10 * total
