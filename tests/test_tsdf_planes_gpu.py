"""Plane finding on the MI355X (csrc/tsdf_planes.hip, go_slam_amd/tsdf_planes.py): the vote and offset histograms equal
tests/tsdf_planes_restatement.py as integer arrays and the moments' rows bit for bit (integer views) on the tilted
wall-and-floor volume, on one cell, on a lattice of prime sizes, with NaN and gradient-free cells planted, at both ends of
the bin and plane ranges and across chunk boundaries; `find_planes`, `floor_plane` and `upright` return what the restated
pipeline returns; only the upright volume has a level slab above its floor; bad arguments are refused without a write; and
an only-tracking run with tsdf.planes and tsdf.upright writes its planes, its transform and an occupancy map."""
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from go_slam_amd import tsdf_planes as TP                      # noqa: E402
import test_tsdf_gpu as TG                                     # noqa: E402  (its lattice and whole run)
import test_tsdf_merge_gpu as MG                               # noqa: E402  (from_dict, same_bits, guarded)
import test_tsdf_planes_cpu as PC                              # noqa: E402  (the tilted scene and the slab's measures)
import tsdf_align_restatement as AR                            # noqa: E402
import tsdf_merge_restatement as MR                            # noqa: E402
import tsdf_planes_restatement as PR                           # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VOXEL = PC.VOXEL
COS2 = float(np.float32(math.cos(math.radians(10.0)) ** 2))
GUARD = MG.GUARD


def chunk():
    return MG.chunk()


def lattice(vol):
    from go_slam_amd import _lib
    return [_lib.ptr(vol.tsdf), _lib.ptr(vol.weight), *vol.dims]


def frame(vol):
    return [float(vol.lo[0]), float(vol.lo[1]), float(vol.lo[2]), vol.voxel]


def raw_votes(vol, bins, min_weight=1.0):
    from go_slam_amd import _lib
    out = torch.zeros((6, bins, bins), dtype=torch.int32, device=DEV)
    rc = _lib.lib().gs_tsdf_plane_votes(*lattice(vol), min_weight, bins, _lib.ptr(out), _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    return rc, out.cpu().numpy().view(np.uint32)


def raw_offsets(vol, normals, o0, bin_m, n_bins, cos2=COS2, min_weight=1.0):
    from go_slam_amd import _lib
    normals, o0 = np.asarray(normals, np.float64).reshape(-1, 3), np.asarray(o0, np.float64).reshape(-1)
    n_d, o_d = torch.as_tensor(normals).to(DEV).contiguous(), torch.as_tensor(o0).to(DEV).contiguous()
    out = torch.zeros((len(normals), n_bins), dtype=torch.int32, device=DEV)
    rc = _lib.lib().gs_tsdf_plane_offsets(*lattice(vol), *frame(vol), min_weight, _lib.ptr(n_d), _lib.ptr(o_d), len(normals),
                                          cos2, bin_m, n_bins, _lib.ptr(out), _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    return rc, out.cpu().numpy().view(np.uint32)


def raw_moments(vol, planes, band, ref, cos2=COS2, min_weight=1.0):
    from go_slam_amd import _lib
    L = _lib.lib()
    planes = np.asarray(planes, np.float64).reshape(-1, 4)
    P = len(planes)
    p_d = torch.as_tensor(planes).to(DEV).contiguous()
    ws = torch.empty(max(L.gs_tsdf_plane_workspace_bytes(P, *vol.dims) // 8, 1), dtype=torch.float64, device=DEV)
    out = torch.full((P, 16), 7.0, dtype=torch.float64, device=DEV)
    rc = L.gs_tsdf_plane_moments(*lattice(vol), *frame(vol), min_weight, _lib.ptr(p_d), P, cos2, band, float(ref[0]),
                                 float(ref[1]), float(ref[2]), _lib.ptr(ws), _lib.ptr(out), _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()


def sixteen_directions(rng, toward):
    """Sixteen unit directions: `toward`'s rows and random ones."""
    extra = rng.normal(size=(16 - len(toward), 3))
    d = np.concatenate([np.asarray(toward, np.float64), extra / np.linalg.norm(extra, axis=1, keepdims=True)])
    return d


@pytest.fixture(scope="module")
def tilted(built_lib):
    """tests/test_tsdf_planes_cpu.py's world tilted by 20 degrees of roll and 10 of pitch, fused on the GPU from the arc
    frames through w2c @ M^-1, and the same lattice as a restated volume (tests/test_tsdf_gpu.py holds the two equal)."""
    M = PC.tilt()
    depth, w2c, mask = PC.arc_inputs(2 * TG.batch() + 1, M)
    vol = TG.volume()
    assert vol.dims == PC.DIMS
    vol.integrate(torch.from_numpy(depth), torch.from_numpy(w2c), TG.INTR, mask=torch.from_numpy(mask))
    d = MG.as_dict(vol, colors=False)
    truth = PC.truth(M)
    return {"M": M, "vol": vol, "d": d, "truth": truth, "up": M[:3, :3] @ np.array([0.0, -1.0, 0.0]),
            "normals": np.stack([truth["wall"][0], truth["floor"][0]])}


def check_histograms(vol, d, normals, o0, bin_m, n_bins, bins=(2, 16, 64)):
    for B in bins:
        ref = PR.votes(d, B)
        rc, out = raw_votes(vol, B)
        assert rc == 0 and out.dtype == ref.dtype and np.array_equal(out, ref), B
    ref = PR.offsets(d, normals, o0, COS2, bin_m, n_bins)
    rc, out = raw_offsets(vol, normals, o0, bin_m, n_bins)
    assert rc == 0 and np.array_equal(out, ref)
    return ref


def test_votes_and_offsets_equal_the_restatement_on_the_tilted_volume(tilted):
    """B = 2, 16 and 64 (two launches over the bins); P = 0, 1, 2 and 16 directions; 2048 bins of 16 directions (three
    launches over the directions)."""
    vol, d = tilted["vol"], tilted["d"]
    n_samples = int(PR.samples(d)["is"].sum())
    votes = PR.votes(d, 16)
    print("samples:", n_samples, "votes per face:", votes.reshape(6, -1).sum(1))
    assert votes.sum() == n_samples > 500
    dirs = sixteen_directions(np.random.default_rng(11), tilted["normals"])
    o0, bin_m, n_bins = TP.offset_bins(d["tsdf"].shape, d["lo"], VOXEL, dirs, VOXEL)
    for P in (1, 2, 16):
        ref = check_histograms(vol, d, dirs[:P], o0[:P], bin_m, n_bins, bins=(2, 16, 64) if P == 1 else ())
        assert ref[0].sum() > 300 and (P < 2 or ref[1].sum() > 100)
    rc, none = raw_offsets(vol, dirs[:0], o0[:0], bin_m, n_bins)
    assert rc == 0 and none.shape == (0, n_bins)
    fine = float(np.float32(VOXEL / 16))                        # 2048 bins of 1 / 16 voxel
    last, o_last = dirs.copy(), o0 + 0.3
    last[14:], o_last[14:] = dirs[:2], o_last[:2]               # the wall and the floor again, in the third launch
    ref = PR.offsets(d, last, o_last, COS2, fine, 2048)
    rc, out = raw_offsets(vol, last, o_last, fine, 2048)
    print("2048 bins:", ref.sum(1))
    assert rc == 0 and np.array_equal(out, ref) and 0 < ref[0].sum() < n_samples and np.array_equal(ref[14:], ref[:2])
    assert ref[1].sum() > 100
    for kw in (dict(min_weight=3.0), dict(cos2=0.5), dict(cos2=1.0), dict(cos2=0.0)):
        kv = {k: v for k, v in kw.items() if k == "min_weight"}
        ref = PR.offsets(d, dirs[:2], o0[:2], kw.get("cos2", COS2), bin_m, n_bins, **kv)
        rc, out = raw_offsets(vol, dirs[:2], o0[:2], bin_m, n_bins, **kw)
        assert rc == 0 and np.array_equal(out, ref), kw
    assert np.array_equal(raw_votes(vol, 16, min_weight=3.0)[1], PR.votes(d, 16, min_weight=3.0))


def planted(dims, seed, voxel=VOXEL):
    """A lattice with a tilted plane through its middle, a little noise, and NaN values, NaN weights, unseen points,
    saturated values and gradient-free saddles planted where the plane passes."""
    rng = np.random.default_rng(seed)
    lo = np.array([-0.3, 0.2, 1.0])
    n = AR.rotation((0.35, -0.25, 0.1)) @ np.array([0.0, 0.0, 1.0])
    ax = [lo[a] + voxel * np.arange(dims[a], dtype=np.float64) for a in range(3)]
    P = np.stack(np.meshgrid(*ax, indexing="ij"), -1)
    o = float(n @ (lo + 0.5 * voxel * (np.asarray(dims) - 1)))
    tsdf = np.clip((P @ n - o) / (4 * voxel) + rng.uniform(-0.02, 0.02, dims), -1.0, 1.0)
    weight = rng.integers(1, 5, dims).astype(np.float64)
    if min(dims) > 2:
        flat = np.flatnonzero(np.abs(tsdf) < 0.2)
        picks = rng.choice(flat, size=min(10, len(flat)), replace=False)
        for at, what in zip(picks, ["nan", "wnan", "unseen", "one", "saddle"] * 2):
            i, j, k = np.unravel_index(at, dims)
            if what == "nan":
                tsdf[i, j, k] = math.nan
            elif what == "wnan":
                weight[i, j, k] = math.nan
            elif what == "unseen":
                weight[i, j, k] = 0.0
            elif what == "one":
                tsdf[i, j, k] = 1.0
            else:
                i, j, k = min(i, dims[0] - 2), min(j, dims[1] - 2), min(k, dims[2] - 2)
                ii, jj, kk = np.meshgrid([0, 1], [0, 1], [0, 1], indexing="ij")
                tsdf[i:i + 2, j:j + 2, k:k + 2] = 0.5 * (-1.0) ** (ii + jj + kk)
                weight[i:i + 2, j:j + 2, k:k + 2] = 1.0
    return MR.volume(tsdf, weight, lo, voxel, 4 * voxel), n, o


@pytest.mark.parametrize("dims", [(2, 2, 2), (13, 7, 11), (2, 3, 2)])
def test_small_and_prime_lattices_with_planted_cells(built_lib, dims):
    """One cell; prime sizes with NaN, unseen, saturated and gradient-free cells where the plane passes; two cells."""
    d, n, o = planted(dims, 3)
    vol = MG.from_dict(d)
    s = PR.samples(d)
    print(dims, "samples:", int(s["is"].sum()), "of", len(s["is"]))
    assert s["is"].sum() >= 1 and (min(dims) == 2 or s["is"].sum() < len(s["is"]))
    if dims == (13, 7, 11):
        assert np.isnan(d["tsdf"]).sum() >= 1 and np.isnan(d["weight"]).sum() >= 1 and s["is"].sum() > 30
        saddles = (s["gg"] == 0) & (s["f"] == 0)
        assert saddles.sum() >= 1 and not s["is"][saddles].any()
    dirs = sixteen_directions(np.random.default_rng(5), n[None])
    o0, bin_m, n_bins = TP.offset_bins(dims, d["lo"], VOXEL, dirs, VOXEL / 2)
    for P in (1, 16):
        ref = check_histograms(vol, d, dirs[:P], o0[:P], bin_m, n_bins)
        assert ref[0].sum() >= 1
    ref3 = TP.box_centre32(dims, d["lo"], VOXEL)
    planes = np.concatenate([dirs, np.full((16, 1), o)], 1)
    ref = PR.moments(d, planes, COS2, VOXEL, ref3, chunk())
    rc, out = raw_moments(vol, planes, VOXEL, ref3)
    assert rc == 0 and MG.same_bits(out, ref) and ref[0, 10] >= 1 and np.isfinite(ref).all()


def test_moments_rows_equal_the_restatement_bit_for_bit(tilted):
    """Sixteen planes in four workgroup groups, five (a full group and one more), one: a plane's row is the same bits in
    each, and in a second run."""
    vol, d = tilted["vol"], tilted["d"]
    rng = np.random.default_rng(13)
    dirs = sixteen_directions(rng, tilted["normals"])
    offs = np.array([tilted["truth"]["wall"][1], tilted["truth"]["floor"][1]] + list(rng.uniform(-4, 4, 14)))
    planes = np.concatenate([dirs, offs[:, None]], 1)
    planes[2:4] = planes[:2] + [0.02, -0.01, 0.015, 0.03]      # near the truth, not on it (rounded to fp32 by the kernel)
    ref3 = TP.box_centre32(d["tsdf"].shape, d["lo"], VOXEL)
    ref = PR.moments(d, planes, COS2, VOXEL, ref3, chunk())
    print("inliers:", ref[:, 10], "agreeing:", ref[:, 11])
    assert ref[0, 10] > 300 and ref[1, 10] > 100 and (ref[:4, 10] <= ref[:4, 11]).all() and not ref[:, 12:].any()
    rc, out = raw_moments(vol, planes, VOXEL, ref3)
    assert rc == 0 and MG.same_bits(out, ref)
    assert MG.same_bits(raw_moments(vol, planes, VOXEL, ref3)[1], out)
    rc, five = raw_moments(vol, planes[:5], VOXEL, ref3)
    assert rc == 0 and MG.same_bits(five, ref[:5])
    for j in (0, 1, 4):
        rc, one = raw_moments(vol, planes[j:j + 1], VOXEL, ref3)
        assert rc == 0 and MG.same_bits(one, ref[j:j + 1]) and MG.same_bits(one, five[j:j + 1])
    for kw, band in ((dict(min_weight=3.0), VOXEL), (dict(cos2=0.5), VOXEL), (dict(), 0.0), (dict(), 4 * VOXEL)):
        kv = {k: v for k, v in kw.items() if k == "min_weight"}
        want = PR.moments(d, planes[:4], kw.get("cos2", COS2), band, ref3, chunk(), **kv)
        rc, got = raw_moments(vol, planes[:4], band, ref3, **kw)
        assert rc == 0 and MG.same_bits(got, want), (kw, band)


@pytest.mark.parametrize("offset", [-1, 0, 1])
def test_moments_across_a_chunk_boundary(built_lib, offset):
    """Lattices of exactly chunk - 1, chunk and chunk + 1 cells, and of a chunk more: the last chunk holds all its cells
    but one, all of them, or a single one (the thin lattices' last cell is a sample)."""
    C = chunk()
    assert C == 2048
    cases = {-1: [(2, 24, 90), (6, 8, 118)],                    # 23 * 89 and 5 * 7 * 117 cells
             0: [(9, 17, 17), (17, 17, 17)],                    # 8 * 16 * 16 and 16^3
             1: [(2, 4, 684), (2, 18, 242)]}[offset]            # 3 * 683 and 17 * 241
    for k, dm in enumerate(cases):
        cells = (dm[0] - 1) * (dm[1] - 1) * (dm[2] - 1)
        assert cells == (k + 1) * C + offset
        n = np.full(3, 0.0005)                                  # nearly square to the shortest axis, through the middle
        n[int(np.argmin(dm))] = 1.0
        n /= np.linalg.norm(n)
        voxel = 0.03125
        ax = [voxel * np.arange(dm[a], dtype=np.float64) for a in range(3)]
        P = np.stack(np.meshgrid(*ax, indexing="ij"), -1)
        o = float(n @ (0.5 * voxel * (np.asarray(dm) - 1)))
        rng = np.random.default_rng(29 + offset)
        d = MR.volume(np.clip((P @ n - o) / (4 * voxel) + rng.uniform(-0.01, 0.01, dm), -1, 1), np.ones(dm), np.zeros(3),
                      voxel, 4 * voxel)
        vol = MG.from_dict(d)
        s = PR.samples(d)
        ref3 = TP.box_centre32(dm, d["lo"], voxel)
        planes = np.array([[*n, o], [*n, o + 0.3 * voxel]])
        ref = PR.moments(d, planes, COS2, voxel, ref3, C)
        print(dm, cells, "cells,", int(s["is"].sum()), "samples, the last cell a sample:", bool(s["is"][-1]), "inliers", ref[:, 10])
        assert ref[0, 10] > 100 and (min(dm) > 2 or s["is"].all())
        rc, out = raw_moments(vol, planes, voxel, ref3)
        assert rc == 0 and MG.same_bits(out, ref)
        assert np.array_equal(raw_votes(vol, 16)[1], PR.votes(d, 16))


# ---- the pipeline -------------------------------------------------------------------------------------------------------
def test_find_planes_floor_and_upright_equal_the_restated_pipeline(tilted):
    vol, d = tilted["vol"], tilted["d"]
    ref = PR.find_planes(d, chunk())
    planes = vol.find_planes()
    print(TP.planes_text(planes))
    assert len(planes) == len(ref) == 2 and TP.planes_text(planes) == TP.planes_text(ref)      # repr(): bit for bit
    for p, q in zip(planes, ref):
        assert p["count"] == q["count"] and MG.same_bits(p["normal"], q["normal"]) and MG.same_bits(p["centroid"], q["centroid"])
    for name, (n, o) in tilted["truth"].items():               # the CPU suite's bounds, on the GPU's planes
        best = max(planes, key=lambda p: float(p["normal"] @ n))
        L = PC.shorter_side(PC.plane_points(d, n, o), n)
        assert math.acos(min(1.0, float(best["normal"] @ n))) <= math.atan(VOXEL / L) and abs(best["offset"] - o) <= VOXEL
    floor = TP.floor_plane(planes, tilted["up"])
    assert floor is planes[1] and float(floor["normal"] @ tilted["truth"]["floor"][0]) > 0.999
    for kw in (dict(bins=8, cone_deg=15.0), dict(min_weight=3.0, iterations=1), dict(band=2 * VOXEL, max_planes=1),
               dict(min_cells=400)):
        assert TP.planes_text(vol.find_planes(**kw)) == TP.planes_text(PR.find_planes(d, chunk(), **kw)), kw
    assert len(vol.find_planes(max_planes=1)) == 1 and len(vol.find_planes(min_cells=400)) == 1
    assert TG.volume().find_planes() == []                      # an empty volume has no plane

    for heading in (None, "walls"):
        up, T = vol.upright(up_hint=tilted["up"], heading=heading)
        T_ref = TP.upright_transform(ref[1], 2, 1, ref[0] if heading else None)
        assert MG.same_bits(T, T_ref) and up.voxel == vol.voxel and up.trunc == vol.trunc
        dims, lo = PR.upright_lattice(d, T_ref)
        assert up.dims == dims and MG.same_bits(up.lo, lo)
        want = PR.upright(d, T_ref)
        assert np.array_equal(TG.bits(up.tsdf), TG.bits(want["tsdf"])) and np.array_equal(TG.bits(up.weight), TG.bits(want["weight"]))
        assert 0.02 < want["touched"].mean() < 0.9
    given, T2 = vol.upright(plane=planes[1], heading="walls")   # a given plane: the same map
    assert MG.same_bits(T2, T) and np.array_equal(TG.bits(given.tsdf), TG.bits(up.tsdf))
    y_up, T3 = vol.upright(plane=planes[1], up_axis=1, up_sign=-1, voxel_size=0.25)
    assert y_up.voxel == 0.25 and np.abs(T3[:3, :3] @ planes[1]["normal"] - [0, -1, 0]).max() < 1e-12
    with pytest.raises(ValueError, match="no floor"):
        vol.upright(up_hint=-tilted["up"])


def test_only_the_upright_volume_has_a_level_slab(tilted):
    """ESDF.occupancy_slice(up_axis=2, height=(0.2, 1.0)) on the upright volume: no column of the floor's area occupied,
    the wall one straight band.  The slab the same distance above the floor along any lattice axis of the tilted volume
    shows more than a third of the floor's own columns occupied."""
    vol, d = tilted["vol"], tilted["d"]
    planes = vol.find_planes()
    wall, floor = planes
    for axis in range(3):
        sign = 1.0 if floor["normal"][axis] > 0 else -1.0
        h = sorted(floor["centroid"][axis] + sign * s for s in PC.SLAB)
        cells = vol.esdf().occupancy_slice(up_axis=axis, height=h)["cells"].cpu().numpy()
        assert np.array_equal(cells, PC.slab_cells(d, axis, *h))
        fp = PC.footprint(d["lo"], d["tsdf"].shape, VOXEL, PC.floor_area_points(d, floor, wall), axis)
        share = float((cells[fp] == 0).mean())
        print(f"tilted, lattice axis {axis}: {share:.3f} of {int(fp.sum())} floor columns occupied")
        assert fp.sum() > 50 and share > 1 / 3
    up, T = vol.upright(up_hint=tilted["up"], heading="walls")
    cells = up.esdf().occupancy_slice(up_axis=2, height=PC.SLAB)["cells"].cpu().numpy()
    pts = PC.floor_area_points(d, floor, wall) @ T[:3, :3].T + T[:3, 3]
    PC.assert_upright_map(cells, PC.footprint(up.lo, up.dims, VOXEL, pts, 2))
    found = up.find_planes()                                    # the upright volume's own wall stands on a lattice axis
    print("the upright volume's planes:", [(p["normal"].round(4).tolist(), round(p["offset"], 4), p["count"]) for p in found])
    assert found[0]["normal"][1] < -0.999 and abs(found[0]["normal"][0]) < 1e-3 and abs(found[0]["normal"][2]) < 0.02


# ---- the C ABI's refusals ---------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_without_a_write(tilted):
    from go_slam_amd import _lib
    L = _lib.lib()
    vol = tilted["vol"]
    fill = 7
    v_buf, votes = MG.guarded(6 * 16 * 16, fill, torch.int32)
    h_buf, hist = MG.guarded(2 * 64, fill, torch.int32)
    o_buf, out = MG.guarded(2 * 16, 7.0, torch.float64)
    ws_buf, ws = MG.guarded(L.gs_tsdf_plane_workspace_bytes(2, *vol.dims) // 8, 7.0, torch.float64)
    normals = torch.as_tensor(tilted["normals"].copy()).to(DEV).contiguous()
    o0 = torch.as_tensor(np.array([-8.0, -8.0])).to(DEV)
    planes = torch.as_tensor(np.concatenate([tilted["normals"], [[-4.0], [-1.2]]], 1)).to(DEV).contiguous()
    names = ("tsdf", "weight", "nx", "ny", "nz")
    base = dict(zip(names, [vol.tsdf, vol.weight, *vol.dims]))
    fr = dict(zip(("lox", "loy", "loz", "voxel"), frame(vol)))

    def arg(v):
        return _lib.ptr(v) if isinstance(v, torch.Tensor) or v is None else v

    def call(fn, order, good, **bad):
        a = dict(good, **bad)
        rc = fn(*[arg(a[k]) for k in order], _lib.stream_ptr(DEV))
        torch.cuda.synchronize()
        return rc

    sizes = [dict(nx=1), dict(ny=1025), dict(nz=0), dict(nx=-5), dict(tsdf=None), dict(weight=None),
             dict(min_weight=math.nan), dict(min_weight=math.inf)]
    frames = [dict(lox=math.nan), dict(loz=math.inf), dict(voxel=0.0), dict(voxel=-1.0), dict(voxel=math.nan), dict(voxel=math.inf)]
    cones = [dict(cos2=-0.1), dict(cos2=1.5), dict(cos2=math.nan)]

    v_good = dict(base, min_weight=1.0, bins=16, votes=votes)
    v_order = list(names) + ["min_weight", "bins", "votes"]
    for bad in sizes + [dict(bins=0), dict(bins=15), dict(bins=66), dict(bins=-2), dict(votes=None)]:
        assert call(L.gs_tsdf_plane_votes, v_order, v_good, **bad) == -1, bad
        assert L.gs_last_error().startswith(b"tsdf_plane_votes"), bad
    assert bool((v_buf == fill).all())

    o_good = dict(base, **fr, min_weight=1.0, normals=normals, o0=o0, P=2, cos2=COS2, bin=0.25, n_bins=64, hist=hist)
    o_order = list(names) + ["lox", "loy", "loz", "voxel", "min_weight", "normals", "o0", "P", "cos2", "bin", "n_bins", "hist"]
    for bad in sizes + frames + cones + [dict(P=-1), dict(P=17), dict(n_bins=0), dict(n_bins=2049), dict(bin=0.0),
                                         dict(bin=-1.0), dict(bin=math.nan), dict(bin=math.inf), dict(normals=None),
                                         dict(o0=None), dict(hist=None)]:
        assert call(L.gs_tsdf_plane_offsets, o_order, o_good, **bad) == -1, bad
        assert L.gs_last_error().startswith(b"tsdf_plane_offsets"), bad
    assert call(L.gs_tsdf_plane_offsets, o_order, o_good, P=0) == 0          # nothing to do, nothing launched
    assert bool((h_buf == fill).all())

    m_good = dict(base, **fr, min_weight=1.0, planes=planes, P=2, cos2=COS2, band=VOXEL, rx=0.75, ry=0.5, rz=2.3, ws=ws, out=out)
    m_order = list(names) + ["lox", "loy", "loz", "voxel", "min_weight", "planes", "P", "cos2", "band", "rx", "ry", "rz", "ws", "out"]
    for bad in sizes + frames + cones + [dict(P=-1), dict(P=17), dict(band=-0.1), dict(band=math.nan), dict(band=math.inf),
                                         dict(rx=math.nan), dict(rz=math.inf), dict(planes=None), dict(ws=None), dict(out=None)]:
        assert call(L.gs_tsdf_plane_moments, m_order, m_good, **bad) == -1, bad
        assert L.gs_last_error().startswith(b"tsdf_plane_moments"), bad
    assert call(L.gs_tsdf_plane_moments, m_order, m_good, P=0) == 0
    assert bool((o_buf == 7.0).all()) and bool((ws_buf == 7.0).all())
    assert L.gs_tsdf_plane_workspace_bytes(-1, *vol.dims) == 0 and L.gs_tsdf_plane_workspace_bytes(17, *vol.dims) == 0
    assert L.gs_tsdf_plane_workspace_bytes(2, 1, 5, 5) == 0
    cells = (vol.dims[0] - 1) * (vol.dims[1] - 1) * (vol.dims[2] - 1)
    assert L.gs_tsdf_plane_workspace_bytes(2, *vol.dims) == 2 * -(-cells // chunk()) * 16 * 8

    # and the good calls write, inside their buffers only (the histograms are added to: the caller zeroes them)
    votes.zero_(), hist.zero_()
    assert call(L.gs_tsdf_plane_votes, v_order, v_good) == 0 and call(L.gs_tsdf_plane_offsets, o_order, o_good) == 0
    assert call(L.gs_tsdf_plane_moments, m_order, m_good) == 0
    assert int(votes.sum()) > 500 and int(hist.sum()) > 300 and bool((out != 7.0).all())
    for buf in (v_buf, h_buf):
        assert bool((buf[:GUARD] == fill).all()) and bool((buf[-GUARD:] == fill).all())
    for buf in (o_buf, ws_buf):
        assert bool((buf[:GUARD] == 7.0).all()) and bool((buf[-GUARD:] == 7.0).all())


# ---- a whole run --------------------------------------------------------------------------------------------------------
def test_a_run_with_planes_and_upright_writes_its_map_in_the_floors_frame(built_lib, tmp_path, monkeypatch):
    """An only-tracking rgbd run with tsdf.planes, tsdf.upright and an occupancy slice: metrics_tsdf_planes.txt holds the
    wall and the floor, map/upright.txt the transform that lays the floor at z = 0, and map/occupancy.pgm is cut 0.2 ..
    1.0 m above it.  The same run without the two keys writes what it wrote before, and nothing else."""
    from go_slam_amd.slam import SLAM
    from go_slam_amd.tsdf import TSDFVolume, load_map
    returned = []
    terminate = SLAM.terminate

    def keeping(self, *args, **kw):
        returned.append(terminate(self, *args, **kw))
        return returned[-1]
    monkeypatch.setattr(SLAM, "terminate", keeping)
    with_dir, without_dir = str(tmp_path / "with"), str(tmp_path / "without")
    base = {"enable": True, "source": "sensor", "voxel_size": 0.1,
            "esdf": {"enable": True, "slice": {"up_axis": 2, "height": [0.2, 1.0]}}}
    TG.whole_run(with_dir, dict(base, planes={"enable": True, "min_cells": 100},
                                upright={"enable": True, "up_hint": "camera", "heading": "walls", "save_volume": True}))
    TG.whole_run(without_dir, dict(base, esdf={"enable": True, "slice": {"up_axis": 1, "height": [0.2, 1.0]}}))
    text = open(f"{with_dir}/metrics_tsdf_planes.txt").read()
    print(text)
    planes, floor = TP.parse_planes(text)
    assert TP.planes_text(planes, None if floor is None else planes[floor]) == text
    stats = returned[0]
    assert stats["tsdf_planes_found"] == len(planes) >= 2 and stats["tsdf_floor_found"] is True and floor is not None
    assert set(returned[0]) - set(returned[1]) == {"tsdf_planes_found", "tsdf_floor_found"}
    # which plane is which: the floor y = 1.2 (y grows downward) and the wall z = 4, as far as this run's poses, tracked
    # by a network that was never trained, put them
    assert planes[floor]["normal"] @ [0.0, -1.0, 0.0] > 0.97 and abs(planes[floor]["offset"] + 1.2) < 0.3
    assert any(p["normal"] @ [0.0, 0.0, -1.0] > 0.97 and abs(p["offset"] + 4.0) < 0.3 for p in planes)
    T = TP.parse_transform(open(f"{with_dir}/map/upright.txt").read())
    assert TP.transform_text(T) == open(f"{with_dir}/map/upright.txt").read()
    assert np.abs(T[:3, :3] @ planes[floor]["normal"] - [0, 0, 1]).max() < 1e-9
    assert abs((T[:3, :3] @ planes[floor]["centroid"] + T[:3, 3])[2]) < 1e-9
    up = TSDFVolume.load(f"{with_dir}/mesh/tsdf_upright_volume.npz", device=DEV)
    assert up.voxel == 0.1 and up.lo[2] < 0 < up.lo[2] + (up.dims[2] - 1) * up.voxel
    grid = load_map(f"{with_dir}/map")
    cells = np.asarray(grid["cells"])
    print("map:", cells.shape, "occupied", int((cells == 0).sum()), "free", int((cells == 254).sum()))
    assert cells.shape == (up.dims[0], up.dims[1]) and (cells == 0).sum() > 20 and (cells == 254).sum() > 200
    new = {"metrics_tsdf_planes.txt", os.path.join("map", "upright.txt"), os.path.join("mesh", "tsdf_upright_volume.npz")}
    assert [p for p in TG.listing(with_dir) if p not in new] == TG.listing(without_dir) and new <= set(TG.listing(with_dir))
    for name in ("mesh/tsdf_mesh.ply", "metrics_traj.txt", "checkpoints/est_poses.npy"):
        assert open(f"{with_dir}/{name}", "rb").read() == open(f"{without_dir}/{name}", "rb").read()
