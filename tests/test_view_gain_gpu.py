"""View gain on the MI355X (csrc/view_gain.hip, go_slam_amd/view.py, ESDF.view_candidates / next_view): every count
equals the serial restatement (tests/view_gain_restatement.py) exactly -- on a random lattice from its corners, faces,
inside and outside, with ray counts around the wave and the workgroup, three ranges and three unknown limits, under the
tight box and the full one; with bits that straddle words, the largest box there is, every lane on one ray and the smallest
lattices; the C ABI refuses bad arguments and writes nothing; the half-seen room of tests/test_frontier_gpu.py is looked
into end to end, as a volume and as a map; and an only-tracking run with tsdf.esdf.next_view ends with map/next_view.txt."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import geodesic_restatement as GR                              # noqa: E402
import test_frontier_gpu as FG                                 # noqa: E402  (its half-seen room and only-tracking run)
import test_view_gain_cpu as VC                                # noqa: E402  (the hand cases)
import view_gain_restatement as VR                             # noqa: E402
from test_frontier_gpu import half_seen_room                   # noqa: E402,F401  (the fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INVALID = -1
DIMS = (9, 11, 70)
RAY_COUNTS = (1, 63, 64, 65, 700)
MANY_RAY_COUNTS = (1025, 2500)                              # above the 1024 lanes of a view's workgroup, the tail ragged
RANGE2 = (1, 50, 10000)
MAX_UNKNOWN = (0, 1, 3)
_REF = {}


def random_state(dims=DIMS, seed=0):
    """About a quarter unknown and a tenth solid (values 2 and above)."""
    p = np.random.default_rng(seed).random(dims)
    return np.where(p < 0.25, 0, np.where(p < 0.35, 2 + (p * 1000).astype(np.int64) % 3, 1)).astype(np.uint8)


def random_views(dims=DIMS, n_inside=40, seed=1):
    """All eight corners, a cell on every face, `n_inside` random cells and two origins outside the lattice."""
    rng = np.random.default_rng(seed)
    top = [n - 1 for n in dims]
    corners = [(a, b, c) for a in (0, top[0]) for b in (0, top[1]) for c in (0, top[2])]
    faces = []
    for a in range(3):
        for side in (0, top[a]):
            c = [int(rng.integers(1, max(top[b], 2))) for b in range(3)]
            c[a] = side
            faces.append(tuple(c))
    inside = [tuple(int(rng.integers(0, n)) for n in dims) for _ in range(n_inside)]
    return np.array(corners + faces + inside + [(-1, 3, 3), (4, 5, dims[2])], dtype=np.int32)


def random_dirs(n=700, seed=2):
    rng = np.random.default_rng(seed)
    d = np.where(rng.random((n, 1)) < 0.35, rng.integers(-6, 7, size=(n, 3)),
                 rng.integers(-VR.MAX_DIR, VR.MAX_DIR + 1, size=(n, 3))).astype(np.int32)
    d[0] = (3, -2, 31000)
    d[5] = 0                                                # casts nothing
    d[6], d[7] = (0, 0, -1), (1, 1, 1)
    return d


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def gpu_gains(state, origins, dirs, range2, max_unknown, box):
    """gs_view_gain itself (range2 need not be a square here): uint32 [V,4], from a buffer that held ones before."""
    from go_slam_amd import _lib
    L = _lib.lib()
    s, o, d = dev(state), dev(np.asarray(origins, dtype=np.int32).reshape(-1, 3)), dev(np.asarray(dirs, dtype=np.int32))
    gain = torch.full((int(o.shape[0]), 4), -1, dtype=torch.int32, device=DEV)
    rc = L.gs_view_gain(_lib.ptr(s), *state.shape, _lib.ptr(o), int(o.shape[0]), _lib.ptr(d), int(d.shape[0]), range2,
                        max_unknown, (ctypes.c_int * 6)(*box), _lib.ptr(gain), _lib.stream_ptr(DEV))
    assert rc == 0, L.gs_last_error()
    return gain.cpu().numpy().view(np.uint32)


def boxes(dims, dirs, range2):
    """(the tight box, the full box) for range2, neither beyond what the lattice allows an offset to be."""
    from go_slam_amd import view
    r = math.isqrt(range2) + (math.isqrt(range2) ** 2 < range2)
    top = [n - 1 for n in dims]
    tight = view.view_box(dirs, r)
    clip = lambda b: tuple(max(b[a], -top[a]) for a in range(3)) + tuple(min(b[3 + a], top[a]) for a in range(3))
    return clip(tight), clip(VR.full_box(r))


@pytest.mark.parametrize("n_rays", RAY_COUNTS)
def test_random_lattice_equals_the_restatement(built_lib, n_rays):
    state, views, dirs = random_state(), random_views(), random_dirs()[:n_rays]
    seen = 0
    for range2 in RANGE2:
        tight, full = boxes(DIMS, dirs, range2)
        for max_unknown in MAX_UNKNOWN:
            want = VR.gains(state, views, dirs, range2, max_unknown)
            assert (want[-2:] == 0).all() and (want[:-2, 3] >= 1).all()          # outside: nothing; inside: the origin
            assert (want[:, :3].sum(axis=1) == want[:, 3]).all()
            seen += int(want[:, 0].sum())
            got = gpu_gains(state, views, dirs, range2, max_unknown, tight)
            assert np.array_equal(got, want), (range2, max_unknown, "tight", tight)
            got = gpu_gains(state, views, dirs, range2, max_unknown, full)
            assert np.array_equal(got, want), (range2, max_unknown, "full", full)
    print("rays", n_rays, "unknown cells counted in all", seen)
    assert seen > 0


@pytest.mark.parametrize("n_rays", MANY_RAY_COUNTS)
def test_a_lane_takes_more_than_one_ray(built_lib, n_rays):
    """More distinct rays than the workgroup has lanes: lane t also casts rays t + 1024 and t + 2048, and the last round
    is ragged.  Fewer views than above keep the restatement to a second or two.  The first 1024 rays never rise along
    the last axis and the later ones all do, so what a lane's second and third ray see, nothing else sees: a kernel that
    dropped or mis-indexed them would miss the counts."""
    state, dirs = random_state(), random_dirs(n=2500, seed=7)
    dirs[:1024, 2] = -np.abs(dirs[:1024, 2])
    dirs[1024:, 2] = np.maximum(np.abs(dirs[1024:, 2]), 1)
    dirs = dirs[:n_rays]
    assert len(np.unique(dirs, axis=0)) >= 0.9 * n_rays     # distinct but for repeats among the small components
    pool = random_views()
    views = np.concatenate([pool[[0, 7, 8, 13]], pool[14:20], pool[-1:]])      # two corners, two faces, six inside, one outside
    differ = 0
    for range2 in RANGE2:
        tight, full = boxes(DIMS, dirs, range2)
        for max_unknown in MAX_UNKNOWN:
            want = VR.gains(state, views, dirs, range2, max_unknown)
            differ += int((want != VR.gains(state, views, dirs[:1024], range2, max_unknown)).any())
            for box in (tight, full):
                assert np.array_equal(gpu_gains(state, views, dirs, range2, max_unknown, box), want), (range2, max_unknown, box)
    hollow = np.where(state > 1, 1, state).astype(np.uint8)  # nothing solid: long walks for every lane's second ray
    want = VR.gains(hollow, views, dirs, 10000, 0)
    differ += int((want != VR.gains(hollow, views, dirs[:1024], 10000, 0)).any())
    assert np.array_equal(gpu_gains(hollow, views, dirs, 10000, 0, boxes(DIMS, dirs, 10000)[0]), want)
    print("rays", n_rays, "cases of 10 in which the rays beyond the first round changed the counts:", differ)
    assert differ >= 4                                      # (at range2 1 a ray's one step need not be along the last axis)


def test_a_direction_outside_the_contract_casts_nothing(built_lib):
    """The C ABI cannot see the directions; the kernel skips one with a component beyond GS_VIEW_MAX_DIR, the most
    negative int included, as the restatement does, and casts the others."""
    state, views = random_state(), random_views(n_inside=8)
    lowest = -0x7fffffff - 1
    bad = [(32768, 0, 0), (0, -32768, 5), (1, 2, lowest), (lowest, lowest, lowest), (0x7fffffff, 1, 1), (65536, 65536, 0),
           (0, 0, lowest)]
    for d in bad:
        assert VR.walk((4, 5, 30), d, DIMS) == []
    nothing = gpu_gains(state, views, bad, 10000, 0, boxes(DIMS, [(1, 1, 1)], 10000)[1])
    assert (nothing == 0).all()
    good = random_dirs()[:20]
    mixed = np.concatenate([np.array(bad[:3], dtype=np.int64), good, np.array(bad[3:], dtype=np.int64)]).astype(np.int32)
    want = VR.gains(state, views, good, 10000, 0)
    assert np.array_equal(VR.gains(state, views, mixed, 10000, 0), want) and want[:-2, 3].min() >= 1
    assert np.array_equal(gpu_gains(state, views, mixed, 10000, 0, boxes(DIMS, good, 10000)[1]), want)


def test_python_entry_point_and_hand_cases(built_lib):
    from go_slam_amd import view
    for name, state, origins, dirs, r, max_unknown, box, want in VC.cases():
        got = view.view_gain(torch.from_numpy(state), origins, dirs, r, max_unknown, box)
        assert got.dtype == torch.int64 and got.is_cuda and got.cpu().tolist() == [list(w) for w in want], name
        got = view.view_gain(dev(state), dev(np.asarray(origins, dtype=np.int32)), torch.tensor(dirs), r, max_unknown, box)
        assert got.cpu().tolist() == [list(w) for w in want], name


def test_bits_that_straddle_words_and_the_largest_box(built_lib):
    from go_slam_amd import _lib
    L = _lib.lib()
    state, views, dirs = random_state(), random_views(n_inside=12), random_dirs()[:65]
    odd = (-3, -2, -5, 3, 4, 5)                             # 7 x 7 x 11 cells: rows of 11 bits
    want = VR.gains(state, views, dirs, 64, 0, odd)
    assert not np.array_equal(want, VR.gains(state, views, dirs, 64, 0))         # the box does clip
    assert np.array_equal(gpu_gains(state, views, dirs, 64, 0, odd), want)
    largest = (-31, -63, -63, 32, 64, 64)                   # 64 x 128 x 128 = GS_VIEW_MAX_BOX_CELLS
    assert 64 * 128 * 128 == VR.MAX_BOX_CELLS
    lds = L.gs_view_gain_lds_bytes((ctypes.c_int * 6)(*largest))
    assert VR.MAX_BOX_CELLS // 8 <= lds <= 160 * 1024
    hollow = np.where(state > 1, 1, state).astype(np.uint8)  # nothing solid: the rays run to the lattice's end
    want = VR.gains(hollow, views, dirs, 10000, 0, largest)
    assert not np.array_equal(want, VR.gains(hollow, views, dirs, 10000, 0))     # axis 2 reaches beyond 64
    assert np.array_equal(gpu_gains(hollow, views, dirs, 10000, 0, largest), want)
    assert np.array_equal(gpu_gains(state, views, dirs, 10000, 3, largest), VR.gains(state, views, dirs, 10000, 3, largest))
    # the small box again: a launch with little LDS after one with the most
    assert np.array_equal(gpu_gains(state, views, dirs, 64, 0, odd), VR.gains(state, views, dirs, 64, 0, odd))


def test_every_lane_on_the_same_ray(built_lib):
    state, views = random_state(), random_views(n_inside=12)
    for d in ((3, -2, 31000), (0, 0, 1), (1, 1, 1), (-5, 2, 4)):
        one = VR.gains(state, views, [d], 10000, 0)
        tight, full = boxes(DIMS, [d], 10000)
        for box in (tight, full):
            assert np.array_equal(gpu_gains(state, views, [d] * 700, 10000, 0, box), one), d
            assert np.array_equal(gpu_gains(state, views, [d], 10000, 0, box), one), d


@pytest.mark.parametrize("dims", [(1, 1, 1), (1, 5, 7)], ids=lambda d: "x".join(map(str, d)))
def test_smallest_lattices_and_no_views(built_lib, dims):
    from go_slam_amd import view
    rng = np.random.default_rng(sum(dims))
    dirs = random_dirs()[:65]
    views = np.array([c for c in np.ndindex(*dims)] + [(0, 0, dims[2]), (-1, 0, 0)], dtype=np.int32)
    for trial in range(3):
        state = rng.integers(0, 3, size=dims).astype(np.uint8)
        for r, max_unknown in ((1, 0), (3, 1), (20, 0)):
            want = VR.gains(state, views, dirs, r * r, max_unknown)
            assert np.array_equal(gpu_gains(state, views, dirs, r * r, max_unknown, VR.full_box(r)), want)
            got = view.view_gain(dev(state), views, dirs, r, max_unknown)
            assert np.array_equal(got.cpu().numpy(), want.astype(np.int64))
    none = view.view_gain(dev(state), np.zeros((0, 3), dtype=np.int32), dirs, 3)
    assert none.shape == (0, 4) and none.dtype == torch.int64
    assert gpu_gains(state, np.zeros((0, 3), dtype=np.int32), dirs, 9, 0, VR.full_box(3)).shape == (0, 4)


def test_c_abi_bad_arguments(built_lib):
    from go_slam_amd import _lib, view
    L = _lib.lib()
    P = _lib.ptr
    stream = _lib.stream_ptr(DEV)
    state_h, views_h, dirs_h = random_state(), random_views(n_inside=4), random_dirs()[:65]
    state, views, dirs = dev(state_h), dev(views_h), dev(dirs_h)
    V, R, GUARD = len(views_h), len(dirs_h), 16
    gain = torch.full((4 * V + 2 * GUARD,), 113, dtype=torch.int32, device=DEV)
    good = (-8, -8, -8, 8, 8, 8)

    def call(s=state, d=DIMS, o=views, v=V, dr=dirs, r=R, range2=64, max_unknown=0, box=good, g=gain):
        return L.gs_view_gain(None if s is None else P(s), *d, None if o is None else P(o), v,
                              None if dr is None else P(dr), r, range2, max_unknown,
                              None if box is None else (ctypes.c_int * 6)(*box), None if g is None else P(g[GUARD:]), stream)

    def lds(box):
        return L.gs_view_gain_lds_bytes(None if box is None else (ctypes.c_int * 6)(*box))
    for bad in ((0, 11, 70), (9, 1025, 70), (9, 11, -1)):
        assert call(d=bad) == INVALID
    assert call(s=None) == INVALID and call(o=None) == INVALID and call(dr=None) == INVALID
    assert call(box=None) == INVALID and call(g=None) == INVALID
    assert call(v=-1) == INVALID and call(r=0) == INVALID and call(r=65537) == INVALID and call(r=-5) == INVALID
    assert call(range2=0) == INVALID and call(range2=-1) == INVALID and call(range2=3 * 1023 ** 2 + 1) == INVALID
    assert call(max_unknown=-1) == INVALID
    over = (0, 0, 0, 16, 61680, 0)                          # 17 x 61681 = 2^20 + 1 cells
    assert 17 * 61681 == VR.MAX_BOX_CELLS + 1
    refused = [over, (1, 0, 0, 2, 2, 2), (0, 0, 0, 3, -1, 3), (-8, -8, 1, 8, 8, 8), (0, 0, -0x7fffffff, 0, 0, 0x7fffffff),
               (-0x7fffffff - 1, 0, 0, 0x7fffffff, 0, 0), (-1023, -1023, -1023, 1023, 1023, 1023)]
    for box in refused:
        assert call(box=box) == INVALID and lds(box) == 0, box
    assert lds(None) == 0
    assert call(v=0, box=over) == INVALID                   # refused whether or not there is work
    assert b"view_gain" in L.gs_last_error()
    with pytest.raises(ValueError, match="at most 1048576"):
        view.view_gain(state, views, dirs_h, 8, box=over)
    torch.cuda.synchronize()
    assert (gain == 113).all()                              # nothing was launched, nothing was written
    accepted = [good, (0, 0, 0, 0, 0, 0), (0, 0, 0, 1023, 1023, 0), (-31, -63, -63, 32, 64, 64), (0, -1048575, 0, 0, 0, 0)]
    sizes = [lds(box) for box in accepted]
    assert all(0 < s <= 160 * 1024 for s in sizes) and sizes[0] >= 17 ** 3 // 8 and sizes[1] < sizes[0] < sizes[2]
    assert sizes[2] == sizes[3] == sizes[4]                 # the cells decide, not the shape
    assert call(v=0) == 0                                   # no views: nothing to do
    torch.cuda.synchronize()
    assert (gain == 113).all()
    for box in accepted:
        gain.fill_(113)
        assert call(box=box) == 0
        torch.cuda.synchronize()
        assert (gain[:GUARD] == 113).all() and (gain[-GUARD:] == 113).all()
        want = VR.gains(state_h, views_h, dirs_h, 64, 0, box)
        assert np.array_equal(gain[GUARD:-GUARD].cpu().numpy().view(np.uint32).reshape(V, 4), want), box
    # the largest range, ray count and limit are accepted
    many = dev(np.tile(dirs_h, (1009, 1))[:65536])
    assert call(dr=many, r=65536, range2=3 * 1023 ** 2, max_unknown=0x7fffffff, box=(-8, -10, -69, 8, 10, 69)) == 0
    torch.cuda.synchronize()
    want = VR.gains(state_h, views_h, dirs_h, 3 * 1023 ** 2, 0)
    assert np.array_equal(gain[GUARD:-GUARD].cpu().numpy().view(np.uint32).reshape(V, 4), want)


# ---- end to end on the half-seen room -----------------------------------------------------------------------------------
VOXEL, ROOM, WALL_X, DOOR_Y, DOOR_Z, START = FG.VOXEL, FG.ROOM, FG.WALL_X, FG.DOOR_Y, FG.DOOR_Z, FG.START
SLAB = (6 * VOXEL, 8 * VOXEL)                               # test_frontiers_on_map_finds_the_same_opening's
CAMERA = {"hfov_deg": 90.0, "vfov_deg": 60.0, "n_u": 12, "n_v": 8, "range_m": 12 * VOXEL, "pitch_deg": 0.0}
N_YAW, STRIDE, RANGE = 8, 4, 12


def room_cost(field):
    """The restated cost field from the start's cell over passable(VOXEL), once."""
    if "room cost" not in _REF:
        passable = field.passable(VOXEL).cpu().numpy()
        _REF["room cost"] = (GR.field(passable != 0, [[8, 6, 30]]), passable)
        _REF["room cost"][0].setflags(write=False)
    return _REF["room cost"]


def restated_table(state, cells, up_axis):
    from go_slam_amd import view
    table = np.zeros((len(cells), N_YAW, 4), dtype=np.int64)
    for j in range(N_YAW):
        dirs = view.ray_directions(CAMERA["hfov_deg"], CAMERA["vfov_deg"], CAMERA["n_u"], CAMERA["n_v"] if up_axis else 1,
                                   2 * math.pi * j / N_YAW, 0.0, up_axis)
        table[:, j] = VR.gains(state, cells, dirs, RANGE * RANGE, 0)
    return table


def test_room_view_candidates_equal_their_restatement(half_seen_room):
    vol, field = half_seen_room
    cost, passable = room_cost(field)
    cells, c, f = field.view_candidates(START, 1, SLAB, robot_radius=VOXEL, stride=STRIDE)
    assert cells.dtype == torch.int32 and c.dtype == torch.int32 and cells.is_cuda and f.start_cell == [8, 6, 30]
    assert np.array_equal(f.cost.cpu().numpy(), cost)
    want_cells, want_cost = VR.candidates(cost, 1, 6, 8, STRIDE, 4096)
    print("candidates", len(want_cells))
    assert len(want_cells) >= 50 and (want_cells[:, 0] <= WALL_X[1]).all()       # on the near side or in the door
    assert np.array_equal(cells.cpu().numpy(), want_cells) and np.array_equal(c.cpu().numpy(), want_cost)
    assert (passable[tuple(want_cells.T)] != 0).all() and (want_cells[:, [0, 2]] % STRIDE == 0).all()
    for stride, cut, height in ((3, 10, SLAB), (1, 4096, (7 * VOXEL, 7 * VOXEL)), (5, 1, (-math.inf, math.inf))):
        a, k0, k1, _, _ = field.slice_arguments(1, height, VOXEL)
        cells, c, _ = field.view_candidates(START, 1, height, robot_radius=VOXEL, stride=stride, max_candidates=cut)
        want_cells, want_cost = VR.candidates(cost, 1, k0, k1, stride, cut)
        assert np.array_equal(cells.cpu().numpy(), want_cells) and np.array_equal(c.cpu().numpy(), want_cost)
    # a start with no passable cell within reach: no candidates, no field
    cells, c, f = field.view_candidates((21 * VOXEL, 6 * VOXEL, 4 * VOXEL), 1, SLAB, robot_radius=VOXEL)
    assert cells.shape == (0, 3) and c.shape == (0,) and f is None


def test_room_next_view_looks_through_the_door(half_seen_room):
    from go_slam_amd import view
    vol, field = half_seen_room
    cost, passable = room_cost(field)
    state = field.state.cpu().numpy()
    res = field.next_view(START, CAMERA, 1, SLAB, n_yaw=N_YAW, robot_radius=VOXEL, stride=STRIDE)
    cells, cell_cost = VR.candidates(cost, 1, 6, 8, STRIDE, 4096)
    table = _REF.setdefault("room table", restated_table(state, cells, 1))
    assert res["n_candidates"] == len(cells) and res["gains"].dtype == torch.int64
    assert np.array_equal(res["gains"].cpu().numpy(), table)                      # the whole gain table
    assert (table[:, :, :3].sum(axis=2) == table[:, :, 3]).all()
    assert (table[:, 3:6, 0] == 0).all() and table[:, :, 0].max() > 0           # heading away from the wall: nothing new
    qualified = table[:, :, 0] >= 1
    assert res["reachable"] and res["n_qualified"] == int(qualified.sum()) >= 1
    assert math.cos(res["yaw"]) > 0 and res["yaw_index"] in (0, 1, 7) and res["yaw"] == 2 * math.pi * res["yaw_index"] / 8
    assert res["gain_cells"] == int(table[:, :, 0][qualified].max())
    lin = [int(np.ravel_multi_index(tuple(c), ROOM)) for c in cells]
    pick, n = view.choose(table, cell_cost, lin, VOXEL)
    v, j = pick[0], pick[1]
    assert res["view_cell"] == cells[v].tolist() and res["yaw_index"] == j and res["score"] == pick[2]
    assert (res["gain_cells"], res["free_cells"], res["solid_cells"]) == tuple(int(x) for x in table[v, j, :3])
    assert res["gain_m3"] == res["gain_cells"] * VOXEL ** 3 == res["score"]
    assert res["view_point"] == [c * VOXEL for c in res["view_cell"]]            # lo = 0
    got = res["cells"].cpu().numpy()
    walk, n = GR.path(cost, passable != 0, tuple(res["view_cell"]), cost.size)
    assert n == len(got) and np.array_equal(got, walk[::-1])                     # the restated walk, reversed
    assert tuple(got[0]) == (8, 6, 30) == tuple(res["start_cell"]) and got[-1].tolist() == res["view_cell"] == res["goal_cell"]
    assert res["length_m"] == float(cell_cost[v]) * VOXEL / 1000.0
    assert res["min_clearance_m"] == float(field.dist.cpu().numpy()[tuple(got.T)].min()) >= VOXEL
    assert np.array_equal(res["points"].cpu().numpy(), got.astype(np.float64) * VOXEL)
    text = view.next_view_text(res)
    back = view.parse_next_view(text)
    assert back["found"] and back["view_cell"] == res["view_cell"] and back["score"] == res["score"]
    # lam: the same table, another score
    far = field.next_view(START, CAMERA, 1, SLAB, n_yaw=N_YAW, robot_radius=VOXEL, stride=STRIDE, lam=2.0)
    pick, _ = view.choose(table, cell_cost, lin, VOXEL, lam=2.0)
    assert far["view_cell"] == cells[pick[0]].tolist() and far["yaw_index"] == pick[1] and far["score"] == pick[2]
    # thresholds above every count: plan's unreachable shape
    none = field.next_view(START, CAMERA, 1, SLAB, n_yaw=N_YAW, robot_radius=VOXEL, stride=STRIDE,
                           min_solid_cells=int(table[:, :, 2].max()) + 1)
    assert none["reachable"] is False and none["view_cell"] is None and none["yaw"] is None and none["n_qualified"] == 0
    assert none["cells"].shape == (0, 3) and none["length_m"] == math.inf and math.isnan(none["min_clearance_m"])
    assert none["n_candidates"] == len(cells) and none["gain_cells"] == 0 and none["start_cell"] == [8, 6, 30]
    assert np.array_equal(none["gains"].cpu().numpy(), table)
    assert view.parse_next_view(view.next_view_text(none))["found"] is False
    # max_unknown reaches the kernel
    few = field.next_view(START, CAMERA, 1, SLAB, n_yaw=2, robot_radius=VOXEL, stride=8, max_unknown=2)
    sub, _ = VR.candidates(cost, 1, 6, 8, 8, 4096)
    for j in range(2):
        dirs = view.ray_directions(90.0, 60.0, 12, 8, math.pi * j, 0.0, 1)
        assert np.array_equal(few["gains"][:, j].cpu().numpy(), VR.gains(state, sub, dirs, RANGE * RANGE, 2).astype(np.int64))


def test_next_view_on_map_looks_through_the_same_door(half_seen_room):
    from go_slam_amd import view
    vol, field = half_seen_room
    grid = field.occupancy_slice(1, SLAB, robot_radius=VOXEL)
    res = view.next_view_on_map(grid, (START[0], START[2]), CAMERA, n_yaw=N_YAW, stride=STRIDE)
    cells = grid["cells"].cpu().numpy()
    state = np.where(cells == 254, 1, np.where(cells == 205, 0, 2)).astype(np.uint8)[None]
    cost = GR.field((cells == 254)[None], [(0, 8, 30)])
    cand, cand_cost = VR.candidates(cost, 0, 0, 0, STRIDE, 4096)
    table = restated_table(state, cand, 0)
    assert res["start_cell"] == (8, 30) and res["n_candidates"] == len(cand) >= 20
    assert np.array_equal(res["gains"].cpu().numpy(), table)
    lin = [int(np.ravel_multi_index(tuple(c), state.shape)) for c in cand]
    pick, n = view.choose(table, cand_cost, lin, VOXEL)
    v, j = pick[0], pick[1]
    assert res["reachable"] and res["view_cell"] == tuple(cand[v][1:].tolist()) and res["yaw_index"] == j
    assert res["n_qualified"] == n and res["gain_cells"] == int(table[v, j, 0]) == int(table[:, :, 0].max()) > 0
    assert math.cos(res["yaw"]) > 0 and res["view_cell"][0] <= WALL_X[1]         # on the near side or in the door
    dirs = view.ray_directions(90.0, 90.0, 12, 1, res["yaw"], 0.0, 0)
    through = [c for d in dirs for c in VR.walk(cand[v], d, state.shape, RANGE * RANGE, None, state)]
    assert any(WALL_X[0] <= c[1] <= WALL_X[1] and DOOR_Z[0] <= c[2] <= DOOR_Z[1] for c in through)     # through the door
    got = res["cells"].cpu().numpy()
    walk, n = GR.path(cost, (cells == 254)[None], tuple(cand[v]), cost.size)
    assert n == len(got) and np.array_equal(got, walk[::-1][:, 1:]) and tuple(got[-1]) == res["view_cell"]
    assert res["length_m"] == float(cand_cost[v]) * VOXEL / 1000.0
    centre = np.array(grid["origin"]) + (got.astype(np.float64) + 0.5) * VOXEL
    assert np.array_equal(res["points"].cpu().numpy(), centre) and res["view_point"] == centre[-1].tolist()
    none = view.next_view_on_map(grid, (START[0], START[2]), CAMERA, n_yaw=N_YAW, stride=STRIDE,
                                 min_gain_cells=int(table[:, :, 0].max()) + 1)
    assert none["reachable"] is False and none["view_cell"] is None and none["cells"].shape == (0, 2)


# ---- whole run ------------------------------------------------------------------------------------------------------
def test_only_tracking_run_ends_with_a_next_view_file(built_lib, tmp_path, monkeypatch):
    from go_slam_amd import plan, view
    from go_slam_amd.slam import SLAM
    returned = []
    terminate = SLAM.terminate

    def keeping(self, *args, **kw):
        returned.append(terminate(self, *args, **kw))
        return returned[-1]
    monkeypatch.setattr(SLAM, "terminate", keeping)
    esdf_cfg = {"enable": True, "max_distance": 1.0,
                "slice": {"up_axis": 1, "height": [-0.5, 0.5], "robot_radius": 0.2}}
    camera = {"hfov_deg": 90.0, "vfov_deg": 60.0, "n_u": 16, "n_v": 12, "range_m": 2.0, "pitch_deg": 0.0}
    with_dir, without_dir = str(tmp_path / "with"), str(tmp_path / "without")
    FG.EG.TG.whole_run(with_dir, {"enable": True, "source": "sensor", "voxel_size": 0.1,
                                  "esdf": {**esdf_cfg, "next_view": {"enable": True, "camera": camera, "up_axis": 1,
                                                                  "height": [-0.5, 0.5], "n_yaw": 4, "robot_radius": 0.2,
                                                                  "stride": 2, "snap": 1.0, "min_gain_cells": 2}}})
    stats = returned[0]
    report = view.parse_next_view(open(f"{with_dir}/map/next_view.txt").read())
    print("map/next_view.txt:", report)
    assert stats["tsdf_next_view_found"] == report["found"] == (report["view_cell"] is not None)
    assert stats["tsdf_next_view_gain_m3"] == report["gain_m3"] == report["gain_cells"] * 0.1 ** 3
    assert stats["tsdf_next_view_candidates"] == report["n_candidates"]
    assert report["found"]                                  # most of this volume was never observed, and the camera fits
    head, points = plan.parse_path(open(f"{with_dir}/map/next_view_path.txt").read())
    assert head["reachable"] and head["length_m"] == report["length_m"] and head["n_points"] == len(points) >= 1
    assert points[-1].tolist() == report["view_point"] and head["min_clearance_m"] >= 0.2
    assert report["gain_cells"] >= 2 and report["n_qualified"] >= 1 and report["score"] == report["gain_m3"]
    assert report["yaw"] == 2 * math.pi * report["yaw_index"] / 4
    extra = [os.path.join("map", "next_view.txt"), os.path.join("map", "next_view_path.txt")]
    FG.EG.TG.whole_run(without_dir, {"enable": True, "source": "sensor", "voxel_size": 0.1, "esdf": esdf_cfg})
    assert not [k for k in returned[1] if "next_view" in k]
    assert set(returned[0]) - set(returned[1]) == {"tsdf_next_view_found", "tsdf_next_view_gain_m3",
                                                   "tsdf_next_view_candidates"}
    listed = FG.EG.TG.listing(with_dir)
    assert all(p in listed for p in extra)
    assert [p for p in listed if p not in extra] == FG.EG.TG.listing(without_dir)
