"""Objects on the MI355X (csrc/tsdf_objects.hip, go_slam_amd/tsdf_objects.py): kind, label, counts, the labels' fixed point,
every table column and the extents (as uint32) equal tests/tsdf_objects_restatement.py exactly on the tilted room, on one
cell, on a lattice of prime sizes with NaN, unseen, saturated and gradient-free cells planted, with 0, 1, 2 and 16 planes, on
cell lattices around the brick's size and around one block of the lattice-wide passes, on a thin diagonal rod through many
bricks and on hand-made label lattices whose clusters meet across a cell corner or miss by one cell; two runs agree;
`find_objects` returns the restated pipeline's boxes bit for bit; a table of fewer rows than clusters writes nothing past
them; bad arguments are refused without a write; and an only-tracking run with tsdf.objects writes a map/objects.txt."""
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from go_slam_amd import tsdf_objects as TO                     # noqa: E402
from go_slam_amd import tsdf_planes as TP                      # noqa: E402
import test_tsdf_gpu as TG                                     # noqa: E402  (its whole run)
import test_tsdf_merge_gpu as MG                               # noqa: E402  (from_dict, guarded)
import test_tsdf_objects_cpu as OC                             # noqa: E402  (the room)
import test_tsdf_planes_cpu as PC                              # noqa: E402
import test_tsdf_planes_gpu as PG                              # noqa: E402  (planted)
import tsdf_merge_restatement as MR                            # noqa: E402
import tsdf_objects_restatement as OR                          # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VOXEL, COS2, GUARD = OC.VOXEL, OC.COS2, MG.GUARD
FILL = 7


def cells_of(vol):
    return tuple(int(n) - 1 for n in vol.dims)


def lattice(vol):
    from go_slam_amd import _lib
    return [_lib.ptr(vol.tsdf), _lib.ptr(vol.weight), *vol.dims, float(vol.lo[0]), float(vol.lo[1]), float(vol.lo[2]), vol.voxel]


def raw_mark(vol, planes, band, cos2=COS2, min_weight=1.0):
    """gs_tsdf_object_mark on fresh buffers -> (rc, kind, label, counts, flags), the first four on the host."""
    from go_slam_amd import _lib
    L = _lib.lib()
    cells = cells_of(vol)
    planes = np.asarray(planes, np.float64).reshape(-1, 4)
    p_d = torch.as_tensor(planes).to(DEV).contiguous()
    kind = torch.full(cells, FILL, dtype=torch.uint8, device=DEV)
    label = torch.full(cells, FILL, dtype=torch.int32, device=DEV)
    counts = torch.full((4,), FILL, dtype=torch.int32, device=DEV)
    flags = torch.full((L.gs_frontier_flags_bytes(*cells),), FILL, dtype=torch.uint8, device=DEV)
    rc = L.gs_tsdf_object_mark(*lattice(vol), min_weight, _lib.ptr(p_d), len(planes), cos2, band, _lib.ptr(kind),
                               _lib.ptr(label), _lib.ptr(counts), _lib.ptr(flags), _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    return rc, kind, label, counts.cpu().numpy().view(np.uint32), flags


def relax(label, flags, max_sweeps=65536):
    """gs_frontier_relax to the fixed point, in place -> the number of sweeps."""
    from go_slam_amd import _lib
    from go_slam_amd import plan
    L = _lib.lib()
    changed = torch.empty(plan.SWEEP_BATCH, dtype=torch.int32, device=DEV)
    return plan.sweep_to_fixed_point(
        lambda s0, k: _lib.check(L.gs_frontier_relax(*label.shape, _lib.ptr(label), _lib.ptr(flags), s0, k, _lib.ptr(changed),
                                                     _lib.stream_ptr(DEV)), "relax"), changed, max_sweeps, "relax")


COLUMNS = (("root", torch.int32, 1), ("size", torch.int32, 1), ("sum", torch.int64, 3), ("sum2", torch.int64, 6),
           ("bbox", torch.int32, 6), ("touch", torch.int32, 1))


def raw_table(kind, label, rows=None):
    """gs_frontier_roots and gs_tsdf_object_table into guard-padded columns of capacity K -> (rc, K, columns on the host,
    their padded buffers, the device root column)."""
    from go_slam_amd import _lib
    L = _lib.lib()
    cells = tuple(label.shape)
    ws_bytes = L.gs_frontier_workspace_bytes(*cells)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    n_roots = torch.empty(1, dtype=torch.int32, device=DEV)
    _lib.check(L.gs_frontier_roots(_lib.ptr(label), *cells, _lib.ptr(ws), ws_bytes, _lib.ptr(n_roots), _lib.stream_ptr(DEV)), "roots")
    K = int(n_roots.item())
    bufs, cols = {}, {}
    for name, dtype, width in COLUMNS:
        bufs[name], flat = MG.guarded(K * width, FILL, dtype)
        cols[name] = flat
    rc = L.gs_tsdf_object_table(_lib.ptr(kind), _lib.ptr(label), *cells, _lib.ptr(ws), ws_bytes, K if rows is None else rows, K,
                                *[_lib.ptr(cols[n]) for n, _, _ in COLUMNS], _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    host = {n: cols[n].cpu().numpy().reshape((K, w) if w > 1 else (K,)) for n, _, w in COLUMNS}
    host["touch"] = host["touch"].view(np.uint32)
    return rc, K, host, bufs, cols["root"]


def raw_extents(vol, label, root, rows, axes, min_weight=1.0):
    from go_slam_amd import _lib
    a_d = torch.as_tensor(np.ascontiguousarray(axes, np.float64)).to(DEV)
    buf, ext = MG.guarded(rows * 6, FILL, torch.int32)
    rc = _lib.lib().gs_tsdf_object_extents(*lattice(vol), min_weight, _lib.ptr(label), _lib.ptr(root), rows, _lib.ptr(a_d),
                                           _lib.ptr(ext), _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == FILL).all()) and bool((buf[-GUARD:] == FILL).all())
    return rc, ext.cpu().numpy().view(np.uint32).reshape(rows, 3, 2)


def guards_hold(bufs):
    return all(bool((b[:GUARD] == FILL).all()) and bool((b[-GUARD:] == FILL).all()) for b in bufs.values())


def same_table(host, ref, rows=None):
    for name, _, _ in COLUMNS:
        got = host[name] if rows is None else host[name][:rows]
        assert got.dtype == ref[name].dtype and np.array_equal(got, ref[name]), name


def expected_flags(obj_cells, cells, b):
    """Flag buffer 0 after the mark: 1 on every brick that holds an object cell; buffer 1: clear."""
    nb = [-(-cells[a] // b[a]) for a in range(3)]
    out = np.zeros(nb, np.uint8)
    at = np.argwhere(obj_cells)
    out[at[:, 0] // b[0], at[:, 1] // b[1], at[:, 2] // b[2]] = 1
    return np.concatenate([out.reshape(-1), np.zeros(out.size, np.uint8)])


def check_all(d, planes, band=VOXEL, cos2=COS2, min_weight=1.0, seed=0):
    """Every stage on the volume dict `d` against the restatement, exactly.  -> what the GPU gave, for comparisons between
    runs, and the number of sweeps."""
    from go_slam_amd import frontier
    vol = MG.from_dict(d)
    ref = OR.mark(d, planes, cos2, band, min_weight=min_weight)
    rc, kind, label, counts, flags = raw_mark(vol, planes, band, cos2, min_weight)
    assert rc == 0
    assert np.array_equal(kind.cpu().numpy(), ref["kind"]) and np.array_equal(label.cpu().numpy(), ref["label"])
    assert counts.tolist() == ref["counts"].tolist()
    assert np.array_equal(flags.cpu().numpy(), expected_flags(ref["kind"] == 1, cells_of(vol), frontier.brick()))
    sweeps = relax(label, flags)
    fixed = OR.labels(ref["label"])
    assert np.array_equal(label.cpu().numpy(), fixed)
    want = OR.table(ref["kind"], fixed)
    rc, K, host, bufs, root = raw_table(kind, label)
    assert rc == 0 and K == len(want["root"]) and guards_hold(bufs)
    same_table(host, want)
    rng = np.random.default_rng(seed)
    axes = rng.normal(size=(K, 3, 3))
    axes[:, 0] = [0.0, -1.0, 0.0]
    ext = np.zeros((0, 3, 2), np.uint32)
    if K:
        rc, ext = raw_extents(vol, label, root, K, axes, min_weight)
        want_ext = OR.extents(d, fixed, want["root"], axes, min_weight=min_weight)
        assert rc == 0 and ext.dtype == want_ext.dtype and np.array_equal(ext, want_ext)
        assert (ext[:, :, 0] <= ext[:, :, 1]).all()             # every cluster has a cell
    return {"kind": kind.cpu().numpy(), "label": label.cpu().numpy(), "counts": counts, "ext": ext, **host}, sweeps, ref


def planes4(planes):
    return np.array([[*p["normal"], p["offset"]] for p in planes], np.float64).reshape(-1, 4)


def sixteen(rng, first):
    extra = rng.normal(size=(16 - len(first), 4))
    extra[:, :3] /= np.linalg.norm(extra[:, :3], axis=1, keepdims=True)
    return np.concatenate([np.asarray(first, np.float64).reshape(-1, 4), extra])


# ---- the kernels against the restatement ------------------------------------------------------------------------------------
def test_the_tilted_room_with_0_1_2_and_16_planes_and_two_runs(built_lib):
    w = OC.world("tilted")
    d = w["vol"]
    assert tuple(n - 1 for n in d["tsdf"].shape) == (36, 20, 69)
    two = planes4(w["structure"])
    all16 = sixteen(np.random.default_rng(5), two)
    for P in (0, 1, 2, 16):
        got, sweeps, ref = check_all(d, all16[:P], seed=P)
        print(f"{P} planes: counts {got['counts'].tolist()}, {len(got['root'])} clusters, {sweeps} sweeps")
        assert got["counts"][0] == 2955 and (P > 0 or got["counts"][1] == 2955)
        if P == 2:
            assert got["counts"].tolist() == [2955, 748, 2207, 49] and sorted(got["size"].tolist())[-3:] == [150, 230, 362]
            again, _, _ = check_all(d, all16[:P], seed=P)
            for key in got:
                assert np.array_equal(got[key], again[key]), key
    for kw in (dict(min_weight=3.0), dict(cos2=0.5), dict(cos2=1.0), dict(cos2=0.0), dict(band=0.0), dict(band=4 * VOXEL)):
        got, _, _ = check_all(d, two, **kw)
        print(kw, got["counts"].tolist())
    shuffled = all16[[5, 1, 0, 9]]                              # the wall before the floor, strangers around them
    got, _, _ = check_all(d, shuffled)
    assert set(np.unique(got["kind"]).tolist()) >= {0, 1, 3, 4}


def test_one_cell(built_lib):
    for planes, kind in (([], 1), ([OC.ON], 2), ([OC.FAR, OC.ON], 3), ([OC.ACROSS, OC.ACROSS2], 2), ([OC.ACROSS], 1)):
        got, _, _ = check_all(PC.one_cell(OC.GOOD), planes, band=0.25)
        assert got["kind"].tolist() == [[[kind]]] and len(got["root"]) == (1 if kind == 1 else 0)
    got, _, _ = check_all(PC.one_cell(np.full(8, 0.25)), [OC.ON], band=0.25)
    assert got["kind"].tolist() == [[[0]]] and got["counts"].tolist() == [0, 0, 0, 0]


def test_prime_sizes_with_planted_cells(built_lib):
    d, n, o = PG.planted((13, 7, 11), 3)
    assert np.isnan(d["tsdf"]).sum() >= 1 and np.isnan(d["weight"]).sum() >= 1
    across = np.cross(n, [0.0, 0.0, 1.0])
    across /= np.linalg.norm(across)
    mid = np.asarray(d["lo"]) + 0.5 * VOXEL * (np.array([13, 7, 11]) - 1)
    for planes in ([], [[*n, o]], [[*across, float(across @ mid)]], [[*across, float(across @ mid)], [*(-across), -float(across @ mid)]]):
        got, sweeps, ref = check_all(d, planes)
        print(len(planes), "planes:", got["counts"].tolist(), len(got["root"]), "clusters", sweeps, "sweeps")
        assert 30 < got["counts"][0] < 12 * 6 * 10
    assert got["counts"][3] > 0                                  # the two-sided plane: a crease of cells that agree with neither


def plane_volume(dims, seed, voxel=0.03125):
    """A plane nearly square to the shortest axis through the lattice's middle, with a little noise: most cells are
    samples, in a few clusters that run through the whole lattice."""
    n = np.full(3, 0.0005)
    n[int(np.argmin(dims))] = 1.0
    n /= np.linalg.norm(n)
    ax = [voxel * np.arange(dims[a], dtype=np.float64) for a in range(3)]
    P = np.stack(np.meshgrid(*ax, indexing="ij"), -1)
    o = float(n @ (0.5 * voxel * (np.asarray(dims) - 1)))
    rng = np.random.default_rng(seed)
    tsdf = np.clip((P @ n - o) / (4 * voxel) + rng.uniform(-0.15, 0.15, dims), -1, 1)
    return MR.volume(tsdf, np.ones(dims), np.zeros(3), voxel, 4 * voxel), n, o


@pytest.mark.parametrize("cells", [(3, 4, 32), (4, 4, 32), (5, 4, 32), (4, 3, 32), (4, 5, 32), (4, 4, 31), (4, 4, 33), (5, 5, 33),
                                   (1, 23, 89), (8, 16, 16), (1, 3, 683)])
def test_cell_lattices_around_the_brick_and_around_one_block(built_lib, cells):
    """One less than, equal to and one more than the brick (4, 4, 32) per axis; 2047, 2048 and 2049 cells: one block of the
    lattice-wide passes less one cell, exactly, and one cell into a second block."""
    from go_slam_amd import frontier
    assert frontier.brick() == (4, 4, 32)
    dims = tuple(c + 1 for c in cells)
    d, n, o = plane_volume(dims, sum(cells))
    for planes, band in (([], d["voxel"]), ([[*n, o]], 0.25 * d["voxel"])):     # the plane itself, a narrow band: many clusters
        got, sweeps, ref = check_all(d, planes, band=band, cos2=0.5)
        print(cells, len(planes), "planes:", got["counts"].tolist(), len(got["root"]), "clusters,", sweeps, "sweeps; the last cell:",
              int(got["kind"].reshape(-1)[-1]))
        assert got["kind"].size == np.prod(cells) and got["counts"][0] >= np.prod(cells) / 10
        if planes:                                              # both kinds, in several clusters that touch the plane
            assert got["counts"][1] >= 8 and got["counts"][2] >= 8 and len(got["root"]) >= 2 and got["touch"].any()


def test_a_thin_diagonal_rod_through_many_bricks(built_lib):
    """A rod of radius 1.3 voxels along the lattice's diagonal: one cluster whose smallest index has to travel through every
    brick on the way, which takes many sweeps and exercises the shortcut label[label[c]]."""
    dims, voxel = (34, 30, 70), 0.05
    ax = [voxel * np.arange(dims[a], dtype=np.float64) for a in range(3)]
    P = np.stack(np.meshgrid(*ax, indexing="ij"), -1)
    a, b = np.array([3.0, 3.0, 3.0]) * voxel, (np.array(dims) - 4.0) * voxel
    t = np.clip(((P - a) @ (b - a)) / float((b - a) @ (b - a)), 0.0, 1.0)
    dist = np.linalg.norm(P - (a + t[..., None] * (b - a)), axis=-1) - 1.3 * voxel
    d = MR.volume(np.clip(dist / (3 * voxel), -1, 1), np.ones(dims), np.zeros(3), voxel, 3 * voxel)
    got, sweeps, ref = check_all(d, [])
    print("rod:", got["counts"].tolist(), len(got["root"]), "clusters,", sweeps, "sweeps, bbox", got["bbox"].tolist())
    assert len(got["root"]) == 1 and got["size"][0] == got["counts"][1] > 500 and sweeps >= 3
    assert (got["bbox"][0, 3:] - got["bbox"][0, :3] >= [25, 21, 60]).all()


def hand_made(kind):
    """gs_frontier_relax / _roots and the table over a hand-made kind lattice (1: object cell; every brick marked)."""
    from go_slam_amd import _lib
    kind = np.ascontiguousarray(kind, np.uint8)
    start = np.where(kind == 1, np.arange(kind.size).reshape(kind.shape), -1).astype(np.int32)
    k_d, label = torch.from_numpy(kind).to(DEV), torch.from_numpy(start).to(DEV)
    n = _lib.lib().gs_frontier_flags_bytes(*kind.shape) // 2
    flags = torch.cat([torch.ones(n, dtype=torch.uint8, device=DEV), torch.zeros(n, dtype=torch.uint8, device=DEV)])
    relax(label, flags)
    fixed = OR.labels(start)
    assert np.array_equal(label.cpu().numpy(), fixed)
    rc, K, host, bufs, _ = raw_table(k_d, label)
    assert rc == 0 and guards_hold(bufs)
    same_table(host, OR.table(kind, fixed))
    return host


def test_clusters_that_meet_across_a_corner_and_clusters_one_cell_apart(built_lib):
    kind = np.zeros((9, 9, 70), np.uint8)
    kind[1:4, 1:4, 28:32] = 1
    kind[4:6, 4:6, 32:35] = 1                                   # meets the first at the corner (3,3,31) - (4,4,32), across bricks
    host = hand_made(kind)
    assert host["size"].tolist() == [36 + 12] and host["bbox"].tolist() == [[1, 1, 28, 5, 5, 34]]
    kind[4:6, 4:6, 32:35] = 0
    kind[5:7, 5:7, 33:36] = 1                                   # one cell of nothing in between, on every axis
    kind[4, 4, 32] = 5                                          # a structure cell there: both touch plane 3, they stay two
    host = hand_made(kind)
    assert host["size"].tolist() == [36, 12] and host["touch"].tolist() == [8, 8]
    kind[4, 4, 32] = 1                                          # an object cell there joins them
    assert hand_made(kind)["size"].tolist() == [49]
    edge = np.zeros((2, 5, 40), np.uint8)                       # touch looks inside the lattice only, at all 26 neighbours
    edge[0, 0, 0], edge[1, 1, 1], edge[1, 4, 39], edge[0, 3, 38], edge[0, 2, 20] = 1, 2, 1, 17, 1
    host = hand_made(edge)
    assert host["size"].tolist() == [1, 1, 1] and host["touch"].tolist() == [1, 0, 1 << 15]


def test_find_objects_equals_the_restated_pipeline_bit_for_bit(built_lib):
    for name in ("tilted", "straight"):
        w = OC.world(name)
        vol = MG.from_dict(w["vol"])
        planes = vol.find_planes()
        assert TP.planes_text(planes) == TP.planes_text(w["planes"])
        floor = TP.floor_plane(planes, w["up"])
        structure, index = TO.structure_planes(planes, floor)
        assert index == w["index"]
        got, ref = vol.find_objects(structure), w["objects"]
        print(name, TO.objects_text(got.boxes))
        assert TO.objects_text(got.boxes) == TO.objects_text(ref.boxes)
        OC.same_boxes(got.boxes, ref.boxes)
        OC.check_boxes(got.boxes, w)
        assert np.array_equal(got.kind.cpu().numpy(), ref.kind) and np.array_equal(got.label.cpu().numpy(), ref.label)
        assert got.counts.tolist() == ref.counts.tolist() and got.n_clusters == ref.n_clusters and got.sweeps >= 1
        for key in ("root", "size", "sum", "sum2", "bbox"):
            assert np.array_equal(getattr(got, key).cpu().numpy(), getattr(ref, key)), key
        assert np.array_equal(got.touch.cpu().numpy().view(np.uint32), ref.touch)
        assert np.array_equal(got.ext, ref.ext) and MG.same_bits(got.axes, ref.axes)
        for kw in (dict(up=w["up"]), dict(min_cells=1, cone_deg=20.0), dict(band=2 * VOXEL, min_weight=0.5)):
            a, b = vol.find_objects(structure, **kw), OR.find_objects(w["vol"], structure, **kw)
            assert TO.objects_text(a.boxes) == TO.objects_text(b.boxes), kw
        bare = vol.find_objects([], up=w["up"])                 # no structure: the surface's connected pieces
        assert TO.objects_text(bare.boxes) == TO.objects_text(OR.find_objects(w["vol"], [], up=w["up"]).boxes)
        assert bare.boxes[0]["cells"] > 2000 and bare.boxes[0]["touches"] == []
    empty = TG.volume().find_objects([], up=[0, -1, 0])         # an empty volume has no object
    assert empty.boxes == [] and empty.n_clusters == 0 and empty.counts.tolist() == [0, 0, 0, 0]


def test_fewer_rows_than_clusters_write_nothing_past_them(built_lib):
    w = OC.world("tilted")
    vol = MG.from_dict(w["vol"])
    two = planes4(w["structure"])
    rc, kind, label, _, flags = raw_mark(vol, two, VOXEL)
    relax(label, flags)
    fixed = label.cpu().numpy()
    for rows in (0, 1, 4):
        rc, K, host, bufs, root = raw_table(kind, label, rows=rows)
        assert rc == 0 and K == 9 and guards_hold(bufs)
        same_table(host, OR.table(kind.cpu().numpy(), fixed, rows=rows), rows=rows)
        for name, _, _ in COLUMNS:
            assert (host[name][rows:].astype(np.int64) == FILL).all(), name
        if rows:
            axes = np.tile(np.eye(3), (rows, 1, 1))
            rc, ext = raw_extents(vol, label, root, rows, axes)
            assert rc == 0 and np.array_equal(ext, OR.extents(w["vol"], fixed, host["root"][:rows], axes))


# ---- the C ABI's refusals ---------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_without_a_write(built_lib):
    from go_slam_amd import _lib
    L = _lib.lib()
    w = OC.world("tilted")
    vol = MG.from_dict(w["vol"])
    cells = cells_of(vol)
    n = int(np.prod(cells))
    bufs = {}
    bufs["kind"], kind = MG.guarded(n, FILL, torch.uint8)
    bufs["label"], label = MG.guarded(n, FILL, torch.int32)
    bufs["counts"], counts = MG.guarded(4, FILL, torch.int32)
    bufs["flags"], flags = MG.guarded(L.gs_frontier_flags_bytes(*cells), FILL, torch.uint8)
    planes = torch.as_tensor(planes4(w["structure"])).to(DEV).contiguous()
    names = ("tsdf", "weight", "nx", "ny", "nz", "lox", "loy", "loz", "voxel", "min_weight")
    base = dict(zip(names, [vol.tsdf, vol.weight, *vol.dims, float(vol.lo[0]), float(vol.lo[1]), float(vol.lo[2]), vol.voxel, 1.0]))

    def arg(v):
        return _lib.ptr(v) if isinstance(v, torch.Tensor) or v is None else v

    def call(fn, order, good, **bad):
        a = dict(good, **bad)
        rc = fn(*[arg(a[k]) for k in order], _lib.stream_ptr(DEV))
        torch.cuda.synchronize()
        return rc

    sizes = [dict(nx=1), dict(ny=1025), dict(nz=0), dict(nx=-5), dict(tsdf=None), dict(weight=None),
             dict(min_weight=math.nan), dict(min_weight=math.inf), dict(lox=math.nan), dict(loz=math.inf), dict(voxel=0.0),
             dict(voxel=-1.0), dict(voxel=math.nan), dict(voxel=math.inf)]
    m_good = dict(base, planes=planes, P=2, cos2=COS2, band=VOXEL, kind=kind, label=label, counts=counts, flags=flags)
    m_order = list(names) + ["planes", "P", "cos2", "band", "kind", "label", "counts", "flags"]
    for bad in sizes + [dict(P=-1), dict(P=17), dict(cos2=-0.1), dict(cos2=1.5), dict(cos2=math.nan), dict(band=-0.1),
                        dict(band=math.nan), dict(band=math.inf), dict(planes=None), dict(kind=None), dict(label=None),
                        dict(counts=None), dict(flags=None)]:
        assert call(L.gs_tsdf_object_mark, m_order, m_good, **bad) == -1, bad
        assert L.gs_last_error().startswith(b"tsdf_object_mark"), bad
    assert all(bool((b == FILL).all()) for b in bufs.values())
    assert call(L.gs_tsdf_object_mark, m_order, m_good) == 0 and guards_hold(bufs)
    ref = OR.mark(w["vol"], planes4(w["structure"]), COS2, VOXEL)
    assert np.array_equal(kind.cpu().numpy().reshape(cells), ref["kind"])
    label3 = label.reshape(cells)
    relax(label3, flags)

    ws_bytes = L.gs_frontier_workspace_bytes(*cells)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    n_roots = torch.empty(1, dtype=torch.int32, device=DEV)
    _lib.check(L.gs_frontier_roots(_lib.ptr(label), *cells, _lib.ptr(ws), ws_bytes, _lib.ptr(n_roots), _lib.stream_ptr(DEV)), "roots")
    K = int(n_roots.item())
    tb, cols = {}, {}
    for name, dtype, width in COLUMNS:
        tb[name], cols[name] = MG.guarded(K * width, FILL, dtype)
    t_good = dict(kind=kind, label=label, cx=cells[0], cy=cells[1], cz=cells[2], ws=ws, ws_bytes=ws_bytes, rows=K, capacity=K, **cols)
    t_order = ["kind", "label", "cx", "cy", "cz", "ws", "ws_bytes", "rows", "capacity"] + [n for n, _, _ in COLUMNS]
    odd = torch.empty(8 * K * 6 + 8, dtype=torch.uint8, device=DEV)[4:]       # an i64 column that is not 8-byte aligned
    for bad in [dict(cx=0), dict(cy=1025), dict(cz=-1), dict(rows=-1), dict(rows=K + 1), dict(capacity=K - 1), dict(ws=None),
                dict(ws_bytes=ws_bytes - 1), dict(ws_bytes=0), dict(kind=None), dict(label=None), dict(sum2=odd), dict(sum=odd)] + \
            [{n: None} for n, _, _ in COLUMNS]:
        assert call(L.gs_tsdf_object_table, t_order, t_good, **bad) == -1, bad
        assert L.gs_last_error().startswith(b"tsdf_object_table"), bad
    assert call(L.gs_tsdf_object_table, t_order, t_good, rows=0) == 0        # nothing to do, nothing launched
    assert all(bool((b == FILL).all()) for b in tb.values())
    assert call(L.gs_tsdf_object_table, t_order, t_good) == 0 and guards_hold(tb)
    assert cols["size"].sum().item() == ref["counts"][1]

    axes = torch.as_tensor(np.tile(np.eye(3), (K, 1, 1))).to(DEV).contiguous()
    e_buf, ext = MG.guarded(K * 6, FILL, torch.int32)
    e_good = dict(base, label=label, root=cols["root"], rows=K, axes=axes, ext=ext)
    e_order = list(names) + ["label", "root", "rows", "axes", "ext"]
    for bad in sizes + [dict(rows=-1), dict(rows=n + 1), dict(label=None), dict(root=None), dict(axes=None), dict(ext=None)]:
        assert call(L.gs_tsdf_object_extents, e_order, e_good, **bad) == -1, bad
        assert L.gs_last_error().startswith(b"tsdf_object_extents"), bad
    assert call(L.gs_tsdf_object_extents, e_order, e_good, rows=0) == 0
    assert bool((e_buf == FILL).all())
    assert call(L.gs_tsdf_object_extents, e_order, e_good) == 0
    assert bool((e_buf[:GUARD] == FILL).all()) and bool((e_buf[-GUARD:] == FILL).all()) and bool((ext != FILL).all())


# ---- a whole run --------------------------------------------------------------------------------------------------------
def test_a_run_with_objects_writes_its_map(built_lib, tmp_path, monkeypatch):
    """An only-tracking rgbd run with tsdf.objects alone, and one with planes, upright and objects: map/objects.txt reads
    back; with upright it holds a second block in the map frame.  The key adds that file and two stats, nothing else."""
    from go_slam_amd.slam import SLAM
    returned = []
    terminate = SLAM.terminate

    def keeping(self, *args, **kw):
        returned.append(terminate(self, *args, **kw))
        return returned[-1]
    monkeypatch.setattr(SLAM, "terminate", keeping)
    alone, both = (str(tmp_path / n) for n in ("alone", "both"))
    base = {"enable": True, "source": "sensor", "voxel_size": 0.1}
    TG.whole_run(alone, dict(base, objects={"enable": True, "min_cells": 4, "min_area_m2": 1.0}))
    TG.whole_run(both, dict(base, planes={"enable": True, "min_cells": 100}, upright={"enable": True, "up_hint": "camera"},
                            objects={"enable": True, "min_cells": 4}))
    for out, stats in ((alone, returned[0]), (both, returned[1])):
        text = open(f"{out}/map/objects.txt").read()
        print(text)
        boxes, moved = TO.parse_objects(text)
        assert TO.objects_text(boxes, moved) == text
        assert stats["tsdf_objects_found"] == len(boxes) and 0 <= stats["tsdf_objects_on_floor"] <= len(boxes)
        assert (moved is not None) == (out == both)
        for b in boxes:
            assert b["cells"] >= 4 and np.abs(b["axes"] @ b["axes"].T - np.eye(3)).max() < 1e-9
    boxes, moved = TO.parse_objects(open(f"{both}/map/objects.txt").read())
    T = TP.parse_transform(open(f"{both}/map/upright.txt").read())
    for b, m in zip(boxes, moved):
        assert np.abs(m["centre"] - (T[:3, :3] @ b["centre"] + T[:3, 3])).max() < 1e-12 and np.abs(m["axes"][0] - [0, 0, 1]).max() < 1e-9
    assert set(returned[1]) - set(returned[0]) == {"tsdf_planes_found", "tsdf_floor_found"}
    assert {"tsdf_objects_found", "tsdf_objects_on_floor"} <= set(returned[0])
    new = {"metrics_tsdf_planes.txt", os.path.join("map", "upright.txt")}
    assert [p for p in TG.listing(both) if p not in new] == TG.listing(alone) and new <= set(TG.listing(both))
    assert os.path.join("map", "objects.txt") in TG.listing(alone) and "metrics_tsdf_planes.txt" not in TG.listing(alone)
    for name in ("mesh/tsdf_mesh.ply", "metrics_traj.txt", "checkpoints/est_poses.npy"):
        assert open(f"{alone}/{name}", "rb").read() == open(f"{both}/{name}", "rb").read()
    with pytest.raises(ValueError, match="tsdf.objects"):      # no poses and no vector: refused before anything is fused
        from go_slam_amd.tsdf import fuse_from_config
        import types
        fuse_from_config(types.SimpleNamespace(cfg={"tsdf": dict(base, objects={"enable": True})}, output=str(tmp_path / "no")))
    assert not os.path.exists(str(tmp_path / "no"))
