"""The distance field on the MI355X (csrc/esdf.hip, TSDFVolume.esdf, ESDF): state, d2 and the bits of dist equal the
serial restatement (tests/esdf_restatement.py) on a fused volume and on synthetic fields at lattice sizes where a
one-lane-per-point, 64-wide kernel can go wrong; query and occupancy_slice equal it bit for bit; a fronto-parallel plane
is recovered to the one voxel the site layers allow; and an only-tracking run with tsdf.esdf ends with
metrics_tsdf_clearance.txt and a map."""
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from go_slam_amd import synth                                  # noqa: E402
import esdf_restatement as ER                                  # noqa: E402
import test_tsdf_gpu as TG                                     # noqa: E402  (its lattice, frames and whole run)
import tsdf_restatement as TR                                  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VOXEL = TG.VOXEL
LO = [b[0] for b in TG.BOUND_EXACT]
H, W = TG.H, TG.W


def bits(t):
    t = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t
    return np.ascontiguousarray(t, dtype=np.float32).view(np.int32)


def assert_field(field, ref):
    assert field.state.dtype == torch.uint8 and field.d2.dtype == torch.int32 and field.dist.dtype == torch.float32
    assert np.array_equal(field.state.cpu().numpy(), ref["state"])
    assert np.array_equal(field.d2.cpu().numpy(), ref["d2"])
    assert np.array_equal(bits(field.dist), bits(ref["dist"]))


def arc_inputs():
    """test_tsdf_gpu.py's arc frames: 5 % zero depth, a random mask, random colours."""
    K = 2 * TG.batch() + 1
    poses = synth.arc_poses(K)
    disp = synth.plane_disps(poses, torch.tensor(TG.INTR), H, W)
    depth = torch.where(disp > 0, 1.0 / disp, torch.zeros_like(disp))
    g = torch.Generator().manual_seed(7)
    depth[torch.rand(K, H, W, generator=g) < 0.05] = 0.0
    mask = (torch.rand(K, H, W, generator=g) > 0.2).float()
    images = torch.rand(K, 3, H, W, generator=g)
    return depth, poses, images, mask


@pytest.fixture(scope="module")
def arc(built_lib):
    """The 37 x 21 x 70 lattice of test_tsdf_gpu.py (a ragged z tail of 6 lanes) fused on the GPU from its arc frames,
    its host copy, and the restatement's fields at R = 3 and R = 1023, min_weight 1 and 2."""
    depth, poses, images, mask = arc_inputs()
    vol = TG.volume()
    assert vol.dims == (37, 21, 70)
    vol.integrate(depth, poses, TG.INTR, images=images, mask=mask)
    host = {k: getattr(vol, k).cpu().numpy().copy() for k in ("tsdf", "weight", "colors")}
    ref = {(R, mw): ER.build(host["tsdf"], host["weight"], R, VOXEL, mw) for R in (3, 1023) for mw in (1.0, 2.0)}
    return types.SimpleNamespace(vol=vol, host=host, ref=ref, frames=(depth, poses, images, mask))


@pytest.mark.parametrize("min_weight", [1.0, 2.0])
@pytest.mark.parametrize("R", [3, 1023])
def test_fused_volume_equals_the_restatement_bit_for_bit(arc, R, min_weight):
    ref = arc.ref[R, min_weight]
    share = [float((ref["state"] == s).mean()) for s in (0, 1, 2)]
    print(f"R {R} min_weight {min_weight}: unknown/free/solid {share}, sites {int(ref['site'].sum())}, "
          f"FAR {int((ref['d2'] == ER.FAR).sum())}")
    assert min(share) > 0.01 and ref["site"].sum() > 100
    assert ((ref["d2"] == ER.FAR).any()) == (R == 3)
    flags = arc.vol.brick_flags()
    field = arc.vol.esdf(None if R == 1023 else R * VOXEL, min_weight=min_weight)
    assert field.radius_voxels == R and field.dims == (37, 21, 70) and field.voxel == VOXEL
    assert np.array_equal(field.lo, np.asarray(LO))
    assert_field(field, ref)
    assert arc.vol._flags is flags                              # the volume is left as it was
    for k in ("tsdf", "weight", "colors"):
        assert np.array_equal(bits(getattr(arc.vol, k)), bits(arc.host[k])), k
    assert not np.array_equal(arc.ref[R, 1.0]["state"], arc.ref[R, 2.0]["state"])


def test_a_snapshot_is_not_changed_by_a_later_integrate(arc):
    depth, poses, images, mask = arc.frames
    vol = TG.volume()
    vol.integrate(depth[:5], poses[:5], TG.INTR, images=images[:5], mask=mask[:5])
    field = vol.esdf(1.0)
    assert field.radius_voxels == 8
    before = [t.cpu().numpy().copy() for t in (field.state, field.d2, field.dist)]
    vol.integrate(depth[5:], poses[5:], TG.INTR, images=images[5:], mask=mask[5:])
    later = vol.esdf(1.0)
    torch.cuda.synchronize()
    for b, t in zip(before, (field.state, field.d2, field.dist)):
        assert np.array_equal(b, t.cpu().numpy())
    assert not np.array_equal(before[1], later.d2.cpu().numpy())
    assert_field(later, ER.build(arc.host["tsdf"], arc.host["weight"], 8, VOXEL))


# ---- synthetic fields -----------------------------------------------------------------------------------------------
def no_site(dims, g):
    """Solid and free halves along the longest axis with a never-seen layer between them: both signs, no site."""
    tsdf, weight = np.ones(dims, np.float32), np.ones(dims, np.float32)
    axis = int(np.argmax(dims))
    sl = [slice(None)] * 3
    if dims[axis] >= 3:
        sl[axis] = slice(0, dims[axis] // 2)
        tsdf[tuple(sl)] = -1.0
        sl[axis] = dims[axis] // 2
        weight[tuple(sl)] = 0.0
    return tsdf, weight


def last_z(dims, g):
    tsdf = np.ones(dims, np.float32)
    tsdf[:, :, -1] = -0.25
    return tsdf, np.ones(dims, np.float32)


def corner(dims, g):
    tsdf = np.ones(dims, np.float32)
    tsdf[0, 0, 0] = -0.25
    return tsdf, np.ones(dims, np.float32)


def random_signs(dims, g):
    tsdf = g.uniform(-1, 1, dims).astype(np.float32)
    weight = (g.random(dims) >= 0.3).astype(np.float32) * 3.0
    tsdf[g.random(dims) < 0.02] = np.nan                       # free where seen
    weight[g.random(dims) < 0.02] = np.nan                     # unknown
    return tsdf, weight


FIELDS = {"no_site": no_site, "last_z": last_z, "corner": corner, "random": random_signs}
# axes shorter than R and than a wave; z lengths at a wave boundary and one past it; several workgroups
LATTICES = [(2, 2, 2), (3, 70, 2), (65, 3, 64), (3, 3, 129), (9, 14, 70)]


def synthetic_volume(dims, tsdf, weight):
    vol = TG.volume([[0.0, (n - 1) * VOXEL] for n in dims], VOXEL)
    assert vol.dims == tuple(dims)
    vol.tsdf.copy_(torch.from_numpy(tsdf))
    vol.weight.copy_(torch.from_numpy(weight))
    vol._flags = None
    return vol


@pytest.mark.parametrize("dims", LATTICES, ids=lambda d: "x".join(map(str, d)))
@pytest.mark.parametrize("name", list(FIELDS))
def test_synthetic_fields_equal_the_restatement_bit_for_bit(built_lib, name, dims):
    tsdf, weight = FIELDS[name](dims, np.random.default_rng(sum(dims)))
    vol = synthetic_volume(dims, tsdf, weight)
    for R in (3, 1023):
        ref = ER.build(tsdf, weight, R, VOXEL)
        field = vol.esdf(None if R == 1023 else R * VOXEL)
        assert_field(field, ref)
        d2, dist = field.d2.cpu().numpy(), field.dist.cpu().numpy()
        if name == "no_site":
            cap = np.float32(VOXEL) * np.float32(R)
            assert (d2 == ER.FAR).all() and np.array_equal(dist, np.where(ref["state"] == 2, -cap, cap))
            assert ((dist < 0).any() and (dist > 0).any()) or max(dims) < 3
        elif name == "last_z":
            assert (d2[:, :, -2:] == 0).all() and (dist[:, :, -1] == 0).all() and np.signbit(dist[:, :, -1]).all()
            if dims[2] > 2:
                assert (d2[:, :, :-2] > 0).all()
        elif name == "corner":
            assert int((d2 == 0).sum()) == 4 and d2[0, 0, 0] == 0 and d2[1, 0, 0] == 0 and d2[0, 1, 0] == 0
            far = tuple(n - 1 for n in dims)                   # nearest: the site one step from the corner along an axis
            if R == 1023:
                assert d2[far] == min(sum(f * f for f in far) - 2 * f + 1 for f in far)
        elif tsdf.size > 1000:
            assert ref["site"].mean() > 0.2 and (ref["state"] == 0).mean() > 0.2


def test_bad_arguments_are_refused_before_any_launch(built_lib):
    from go_slam_amd import _lib
    L = _lib.lib()
    x = torch.full((8,), 7.0, device=DEV)
    s = _lib.stream_ptr(DEV)
    for dims in [(1, 2, 2), (2, 1025, 2), (2, 2, 0)]:
        rc = L.gs_esdf_build(_lib.ptr(x), _lib.ptr(x), *dims, 1.0, 3, 0.1, _lib.ptr(x), _lib.ptr(x), _lib.ptr(x), s)
        assert rc == -1 and b"outside [2, 1024]" in L.gs_last_error()
    for radius in (0, 1024, -1):
        rc = L.gs_esdf_build(_lib.ptr(x), _lib.ptr(x), 2, 2, 2, 1.0, radius, 0.1, _lib.ptr(x), _lib.ptr(x), _lib.ptr(x), s)
        assert rc == -1 and b"radius" in L.gs_last_error()
    rc = L.gs_esdf_build(_lib.ptr(x), _lib.ptr(x), 2, 2, 2, 1.0, 3, 0.0, _lib.ptr(x), _lib.ptr(x), _lib.ptr(x), s)
    assert rc == -1 and b"voxel" in L.gs_last_error()
    rc = L.gs_esdf_build(_lib.ptr(x), None, 2, 2, 2, 1.0, 3, 0.1, _lib.ptr(x), _lib.ptr(x), _lib.ptr(x), s)
    assert rc == -1 and b"null" in L.gs_last_error()
    for a, k0, k1 in [(3, 0, 0), (-1, 0, 0), (2, 1, 0), (2, 0, 2), (0, -1, 1)]:
        rc = L.gs_esdf_slice(_lib.ptr(x), _lib.ptr(x), _lib.ptr(x), 2, 2, 2, a, k0, k1, 0, 0, _lib.ptr(x), _lib.ptr(x), s)
        assert rc == -1
    rc = L.gs_esdf_slice(_lib.ptr(x), _lib.ptr(x), _lib.ptr(x), 2, 2, 2, 0, 0, 1, -1, 0, _lib.ptr(x), _lib.ptr(x), s)
    assert rc == -1
    rc = L.gs_esdf_query(_lib.ptr(x), _lib.ptr(x), 2, 2, 2, 0.0, 0.0, 0.0, 0.1, _lib.ptr(x), -1, _lib.ptr(x), _lib.ptr(x),
                         _lib.ptr(x), s)
    assert rc == -1
    rc = L.gs_esdf_query(_lib.ptr(x), _lib.ptr(x), 2, 2, 2, 0.0, 0.0, 0.0, 0.1, None, 0, None, None, None, s)
    assert rc == 0                                              # nothing to do, nothing launched
    torch.cuda.synchronize()
    assert bool((x == 7.0).all())


# ---- query ----------------------------------------------------------------------------------------------------------
def query_points():
    """4096 rows: uniform inside, exact lattice points, a coordinate exactly on the last lattice plane, outside, and
    NaN / +-inf rows.  LO and VOXEL are exact in binary, so lattice points are exact in fp32."""
    g = np.random.default_rng(21)
    dims = np.array([37, 21, 70])
    lo, hi = np.asarray(LO), np.asarray(LO) + (dims - 1) * VOXEL
    inside = g.uniform(lo, hi, (3000, 3))
    lattice = lo + g.integers(0, dims - 1, (500, 3)) * VOXEL
    last = g.uniform(lo, hi, (200, 3))
    last[np.arange(200), g.integers(0, 3, 200)] = 0.0
    last = np.where(last == 0.0, hi, last)
    first = g.uniform(lo, hi, (100, 3))
    first[np.arange(100), g.integers(0, 3, 100)] = np.inf
    first = np.where(np.isinf(first), lo, first)                # on the first plane: valid
    outside = g.uniform(lo - 1.0, hi + 1.0, (200, 3))
    outside[:100, 0] = g.uniform(hi[0] + 1e-3, hi[0] + 2.0, 100)
    outside[100:, 2] = g.uniform(lo[2] - 2.0, lo[2] - 1e-3, 100)
    bad = g.uniform(lo, hi, (96, 3))
    bad[np.arange(96), g.integers(0, 3, 96)] = np.tile([np.nan, np.inf, -np.inf], 32)
    pts = np.concatenate([inside, lattice, last, first, outside, bad]).astype(np.float32)
    assert pts.shape == (4096, 3)
    return pts


def test_query_equals_the_restatement_bit_for_bit(arc):
    from go_slam_amd import _lib
    pts = query_points()
    ref = arc.ref[1023, 1.0]
    d, g, valid, known = ER.query(ref["dist"], ref["state"], LO, VOXEL, pts)
    print(f"valid {int(valid.sum())}, known {int(known.sum())}, negative {int((d < 0).sum())}")
    assert valid[:3000].all() and valid[3000:3500].all() and not valid[3500:3700].any() and valid[3700:3800].all()
    assert not valid[3800:].any() and 500 < known.sum() < valid.sum() and (d[known] < 0).any()
    field = arc.vol.esdf()
    out = field.query(torch.from_numpy(pts))
    assert out["dist"].shape == (4096,) and out["grad"].shape == (4096, 3) and out["valid"].dtype == torch.bool
    assert np.array_equal(out["valid"].cpu().numpy(), valid) and np.array_equal(out["known"].cpu().numpy(), known)
    assert np.array_equal(bits(out["dist"]), bits(d)) and np.array_equal(bits(out["grad"]), bits(g))
    # every output row is written: buffers that start with other bits end with the same results
    dist = torch.full((4096,), 7.0, device=DEV)
    grad = torch.full((4096, 3), 7.0, device=DEV)
    flags = torch.full((4096,), 255, dtype=torch.uint8, device=DEV)
    p = torch.from_numpy(pts).to(DEV)
    rc = _lib.lib().gs_esdf_query(_lib.ptr(field.dist), _lib.ptr(field.state), 37, 21, 70, *[float(v) for v in LO], VOXEL,
                                  _lib.ptr(p), 4096, _lib.ptr(dist), _lib.ptr(grad), _lib.ptr(flags), _lib.stream_ptr(DEV))
    assert rc == 0
    assert np.array_equal(bits(dist), bits(d)) and np.array_equal(bits(grad), bits(g))
    assert np.array_equal(flags.cpu().numpy(), valid.astype(np.uint8) + 2 * known.astype(np.uint8))
    empty = field.query(torch.zeros(0, 3))
    assert empty["dist"].shape == (0,) and empty["grad"].shape == (0, 3)


# ---- occupancy_slice ------------------------------------------------------------------------------------------------
def test_occupancy_slice_equals_the_restatement(arc):
    ref = arc.ref[1023, 1.0]
    field = arc.vol.esdf()
    dims = (37, 21, 70)
    seen = set()
    for a in range(3):
        u, v = [ax for ax in range(3) if ax != a]
        layer = LO[a] + (dims[a] // 2) * VOXEL
        for height, k0, k1 in (((layer, layer), dims[a] // 2, dims[a] // 2), ((-math.inf, math.inf), 0, dims[a] - 1)):
            for radius, occ_d2 in ((0.0, 0), (2.5 * VOXEL, 6)):
                for fraction in (0.0, 0.5, 1.0):
                    args = field.slice_arguments(a, height, radius, fraction)
                    assert args == (a, k0, k1, occ_d2, math.ceil(fraction * (k1 - k0 + 1)))
                    cells, clearance = ER.occupancy_slice(ref["state"], ref["d2"], ref["dist"], *args)
                    out = field.occupancy_slice(a, height, robot_radius=radius, known_fraction=fraction)
                    assert out["axes"] == (u, v) and out["resolution"] == VOXEL
                    assert out["origin"] == (LO[u] - VOXEL / 2, LO[v] - VOXEL / 2)
                    assert out["cells"].shape == (dims[u], dims[v]) and out["cells"].dtype == torch.uint8
                    assert np.array_equal(out["cells"].cpu().numpy(), cells), args
                    assert np.array_equal(bits(out["clearance"]), bits(clearance)), args
                    values = set(np.unique(cells).tolist())
                    assert values <= {0, 205, 254}
                    print(args, {val: int((cells == val).sum()) for val in sorted(values)})
                    if values == {0, 205, 254}:
                        seen.add(args)
    assert (1, 0, 20, 0, 11) in seen        # y up, the whole axis: occupied, free and unknown cells in one map


# ---- the plane scene ------------------------------------------------------------------------------------------------
def test_fronto_parallel_plane_is_recovered_to_a_voxel(built_lib):
    """test_tsdf_gpu.py's plane z = c seen by three unrotated cameras.  Every sign change lies between the two lattice
    layers around the plane, so the sites are those layers and the free one is less than a voxel in front of the plane.
    A free point seen by a camera has the point straight ahead of it on that layer inside the same frustum (the frustum
    of an unrotated camera widens with z), so its distance to the nearest site lies within [c - z - voxel, c - z]: dist
    is within one voxel of the true distance c - z (1e-5 m for the fp32 roundings).  Derived for this axis-aligned
    scene only."""
    c = 2.013
    depth, w2c = TR.plane_scene(c)
    vol = TG.volume(TR.PLANE_BOUND, TR.PLANE_VOXEL)
    vol.integrate(torch.from_numpy(depth), torch.from_numpy(w2c), TR.PLANE_INTR)
    field = vol.esdf()
    state, dist = field.state.cpu().numpy(), field.dist.cpu().numpy().astype(np.float64)
    z = TR.PLANE_BOUND[2, 0] + np.arange(vol.dims[2]) * TR.PLANE_VOXEL
    front = (state == 1) & (z < c)[None, None, :]
    err = np.abs(dist - (c - z)[None, None, :])[front]
    print(f"{int(front.sum())} free points in front of the plane, largest |dist - (c - z)| = {err.max():.6f} m")
    assert front.sum() > 10000
    assert err.max() <= TR.PLANE_VOXEL + 1e-5
    site_layers = np.unique(np.nonzero(field.d2.cpu().numpy() == 0)[2])
    assert site_layers.tolist() == [int(c / TR.PLANE_VOXEL), int(c / TR.PLANE_VOXEL) + 1]


# ---- clearance and a whole run --------------------------------------------------------------------------------------
def test_trajectory_clearance_against_numpy(arc, tmp_path):
    from go_slam_amd import tsdf
    ref = arc.ref[1023, 1.0]
    field = arc.vol.esdf()
    pts = query_points()[::37]
    c2w = np.tile(np.eye(4), (len(pts), 1, 1))
    c2w[:, :3, 3] = pts.astype(np.float64)
    d, _, valid, known = ER.query(ref["dist"], ref["state"], LO, VOXEL, pts)
    ok = valid & known
    assert ok.sum() > 10 and (~ok).sum() > 10 and (d[ok] < 0).any()
    path = str(tmp_path / "metrics_tsdf_clearance.txt")
    res = tsdf.trajectory_clearance(field, [torch.from_numpy(m) for m in c2w], out_path=path)
    assert res["n_poses"] == len(pts) and res["n_unknown"] == int((~ok).sum()) and res["n_inside"] == int((d[ok] < 0).sum())
    assert res["clearance_min_m"] == float(d[ok].min())
    assert abs(res["clearance_mean_m"] - d[ok].astype(np.float64).mean()) <= 1e-12
    assert tsdf.parse_clearance(open(path).read()) == res
    none = tsdf.trajectory_clearance(field, [])
    assert none["n_poses"] == 0 and math.isnan(none["clearance_min_m"]) and math.isnan(none["clearance_mean_m"])


def test_only_tracking_run_ends_with_clearance_and_a_map(built_lib, tmp_path, monkeypatch):
    from go_slam_amd import tsdf
    from go_slam_amd.neus.mesh import load_mesh
    from go_slam_amd.slam import SLAM
    returned = []
    terminate = SLAM.terminate

    def keeping(self, *args, **kw):
        returned.append(terminate(self, *args, **kw))
        return returned[-1]
    monkeypatch.setattr(SLAM, "terminate", keeping)
    out_dir = str(tmp_path / "run")
    TG.whole_run(out_dir, {"enable": True, "source": "sensor", "voxel_size": 0.1,
                           "esdf": {"enable": True, "max_distance": 1.0,
                                    "slice": {"up_axis": 1, "height": [-0.5, 0.5], "robot_radius": 0.2}}})
    stats = returned[0]
    res = tsdf.parse_clearance(open(f"{out_dir}/metrics_tsdf_clearance.txt").read())
    print("metrics_tsdf_clearance.txt:", res)
    assert res["n_poses"] == TG.N_RUN
    assert 0 <= res["n_inside"] <= TG.N_RUN - res["n_unknown"] and 0 <= res["n_unknown"] <= TG.N_RUN
    for key, name in (("tsdf_clearance_min_m", "clearance_min_m"), ("tsdf_clearance_inside", "n_inside"),
                      ("tsdf_clearance_unknown", "n_unknown")):
        assert stats[key] == res[name] or (math.isnan(stats[key]) and math.isnan(res[name]))
    grid = tsdf.load_map(f"{out_dir}/map")
    dims = TR.lattice_dims([[-4.0, 4.0], [-3.0, 2.0], [-1.0, 5.0]], 0.1)
    assert grid["cells"].shape == (dims[0], dims[2]) and grid["resolution"] == 0.1
    assert grid["origin"] == (-4.0 - 0.5 * 0.1, -1.0 - 0.5 * 0.1)
    assert set(np.unique(grid["cells"]).tolist()) <= {0, 205, 254}
    assert not os.path.exists(f"{out_dir}/mesh/tsdf_esdf.npz")
    mesh = load_mesh(f"{out_dir}/mesh/tsdf_mesh.ply")
    assert len(mesh.faces) >= 1
    extra = {"metrics_tsdf_clearance.txt", os.path.join("map", "occupancy.pgm"), os.path.join("map", "occupancy.yaml"),
             os.path.join("mesh", "tsdf_mesh.ply")}
    assert extra <= set(TG.listing(out_dir))
