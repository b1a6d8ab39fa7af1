"""The particle-filter kernels on the MI355X (csrc/mcl.hip, go_slam_amd/mcl.py): move, weigh, estimate and resample equal the
serial restatement (tests/mcl_restatement.py) with torch.equal into sentinel-filled outputs, the C entries refuse bad
arguments before anything is written, two runs give equal bits, `ParticleFilter` tracks the closed loop of
tests/test_mcl_cpu.py within the restatement's recorded error, notices a kidnap and recovers from it, and an only-tracking
run with tsdf.esdf.mcl ends with map/mcl.txt."""
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import mcl_restatement as R                                    # noqa: E402
import scan_restatement as SR                                  # noqa: E402
import test_esdf_gpu as EG                                     # noqa: E402  (its only-tracking run)
import test_mcl_cpu as MC                                      # noqa: E402  (the closed loop's inputs, once)
import test_scan_cpu as SC                                     # noqa: E402  (the recovery scene)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INVALID = -1
MASK64 = (1 << 64) - 1
_REF = {}


def gpu(a):
    a = np.asarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    elif a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(np.array(a, order="C")).to(DEV)   # a copy: the shared references are read-only


def shared(key, make):
    if key not in _REF:
        value = make()
        for a in (value if isinstance(value, tuple) else (value,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _REF[key] = value
    return _REF[key]


MAPS = {"1x1": (1, 1), "9x300": (9, 300), "scene": (48, 40)}


def base_map(name):
    def make():
        if name == "scene":
            return np.array(SC.scene())
        if name == "1x1":
            return np.full((1, 1), 254, dtype=np.uint8)
        return SC.random_map(MAPS[name], sum(MAPS[name]))      # free, unknown, occupied at probability one third each
    return shared(("map", name), make)


def field_of(name, radius=3):
    return shared(("field", name, radius), lambda: SR.field(base_map(name), radius))


def particles_on(name, n, H):
    """int32 [n,3]: the four corners of the map in milli-cells first, then one particle each on a free, an occupied and
    an unknown cell where the map has one, then drawn ones (a third of a drawn map's cells carry a robot)."""
    def make():
        cells = base_map(name)
        n_u, n_v = cells.shape
        rng = np.random.default_rng(n + H)
        rows = [(0, 0, 0), (1000 * n_u - 1, 1000 * n_v - 1, H - 1), (0, 1000 * n_v - 1, H // 2), (1000 * n_u - 1, 0, H // 3)]
        for value in (254, 0, 205):
            at = np.argwhere(cells == value)
            if len(at):
                u, v = at[len(at) // 2]
                rows.append((1000 * int(u) + 999, 1000 * int(v), int(rng.integers(H))))
        rows = rows[:n]
        more = n - len(rows)
        drawn = np.stack([rng.integers(0, 1000 * n_u, more), rng.integers(0, 1000 * n_v, more), rng.integers(0, H, more)], 1)
        return np.concatenate([np.array(rows, dtype=np.int64).reshape(-1, 3), drawn]).astype(np.int32)
    return shared(("particles", name, n, H), make)


SPECIAL_ENDS = [(-1, -1), (-1000, -1001), (-999, 999), (0, 0), (4000000, 0), (4000001, 0), (0, -4000001), (-4000000, -4000000),
                (0x7fffffff, 5), (5, -0x7fffffff), (-500, 500), (-501, 499), (-0x80000000, -0x80000000)]


def ends_for(name, H, B):
    """int32 [H,B,2]: drawn end points within a few cells and across the whole map, with the special ones -- negative sums
    that need the floor, the limit of 4 000 000 and beyond, the ends of 32 bits -- spread over the headings."""
    def make():
        n_u, n_v = MAPS[name]
        rng = np.random.default_rng(H * 4099 + B)
        ends = np.where(rng.random((H, B, 1)) < 0.5, rng.integers(-3000, 3001, (H, B, 2)),
                        rng.integers(-1000 * max(n_u, n_v), 1000 * max(n_u, n_v) + 1, (H, B, 2)))
        for k, e in enumerate(SPECIAL_ENDS):
            ends[k % H, (k // H) % B] = e
        return ends.astype(np.int32)
    return shared(("ends", name, H, B), make)


CASES = [("1x1", 1, 1, 1), ("1x1", 63, 4, 63), ("9x300", 64, 4, 64), ("9x300", 65, 360, 65), ("scene", 257, 360, 300),
         ("scene", 1025, 4, 1), ("scene", 4099, 360, 64), ("9x300", 257, 1, 300)]


# ---- every kernel against the restatement -------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n,H,B", CASES)
def test_move_equals_the_restatement(built_lib, name, n, H, B):
    from go_slam_amd import mcl as M
    shape = MAPS[name]
    parts = particles_on(name, n, H)
    rot = M.heading_table(H)
    rng = np.random.default_rng(n)
    noise = np.stack([rng.integers(-3000, 3001, n), rng.integers(-3000, 3001, n), rng.integers(-2 * H - 3, 2 * H + 4, n)], 1)
    noise[0] = (1 << 20, -(1 << 20), -(1 << 20))
    noise = noise.astype(np.int32)
    for odo in ((1000, 0, 0), (-700, 450, -7), (1 << 20, -(1 << 20), 1 << 20), (0, 0, 0)):
        want = shared(("move", name, n, H, odo), lambda: R.move(parts, rot, noise, odo, shape))
        out = torch.full((n, 3), -77, dtype=torch.int32, device=DEV)
        src = gpu(parts)
        got = M.move(src, rot, noise, odo, shape, out=out)
        assert got is out and torch.equal(out.cpu(), torch.from_numpy(want)), odo
        assert torch.equal(src.cpu(), torch.from_numpy(parts))                      # the input is left alone
        assert M.move(src, rot, noise, odo, shape, out=src) is src and torch.equal(src.cpu(), torch.from_numpy(want))   # in place
    assert int(want[:, 0].min()) >= 0 and int(want[:, 0].max()) < 1000 * shape[0] and int(want[:, 2].max()) < H


@pytest.mark.parametrize("allow_unknown", [False, True])
@pytest.mark.parametrize("name,n,H,B", CASES)
def test_weigh_equals_the_restatement(built_lib, name, n, H, B, allow_unknown):
    from go_slam_amd import mcl as M
    cells, cost = base_map(name), field_of(name)
    parts, ends = particles_on(name, n, H), ends_for(name, H, B)
    want = shared(("weigh", name, n, H, B, allow_unknown), lambda: R.weigh(cost, cells, parts, ends, 10, allow_unknown))
    out = (torch.full((n,), 12345, dtype=torch.int32, device=DEV), torch.full((1,), 999, dtype=torch.int64, device=DEV))
    S, best = M.weigh(gpu(cost), gpu(cells), gpu(parts), ends, 10, allow_unknown, out=out)
    assert S is out[0] and best is out[1]
    assert torch.equal(S.cpu(), torch.from_numpy(want[0].view(np.int32))) and best.item() & MASK64 == want[1]
    again = M.weigh(gpu(cost), gpu(cells), gpu(parts), ends, 10, allow_unknown)     # two runs, equal bits
    assert torch.equal(again[0], S) and torch.equal(again[1], best)
    if name != "1x1" and n >= 64:
        standing = int((want[0] != R.NO_SCORE).sum())
        assert 0 < standing < n
        if name == "9x300":                                                         # unknown cells carry a robot or do not
            other = shared(("weigh", name, n, H, B, not allow_unknown), lambda: R.weigh(cost, cells, parts, ends, 10, not allow_unknown))
            assert (standing > int((other[0] != R.NO_SCORE).sum())) == allow_unknown


def drawn_scores(n, L, seed):
    rng = np.random.default_rng(seed)
    S = rng.integers(40, 40 + 2 * L, n).astype(np.uint32)
    S[rng.random(n) < 0.25] = R.NO_SCORE
    return S


def run_estimate(M, S, parts, rot, lut):
    n = len(S)
    out = (torch.full((n,), -5, dtype=torch.int32, device=DEV), torch.full((n,), -5, dtype=torch.int64, device=DEV),
           torch.full((16,), -5, dtype=torch.int64, device=DEV))
    got = M.estimate(S, gpu(parts), rot, lut, out=out)
    assert all(g is o for g, o in zip(got, out))
    return got


def assert_estimate(got, want):
    w, cum, stats = got
    assert torch.equal(w.cpu(), torch.from_numpy(want[0].view(np.int32)))
    assert torch.equal(cum.cpu(), torch.from_numpy(want[1].view(np.int64)))
    assert [v & MASK64 for v in stats.cpu().tolist()] == want[2]


@pytest.mark.parametrize("n,H", [(1, 1), (63, 4), (64, 360), (65, 360), (257, 4), (1024, 360), (1025, 360), (4099, 360)])
def test_estimate_equals_the_restatement(built_lib, n, H):
    from go_slam_amd import mcl as M
    rot, lut = M.heading_table(H), M.weight_table(60)
    parts = particles_on("scene", n, H)
    S = shared(("scores", n), lambda: drawn_scores(n, len(lut), n))
    if n == 1:
        S = np.array([7], dtype=np.uint32)
    want = shared(("estimate", n, H), lambda: R.estimate(S, parts, rot, lut))
    got = run_estimate(M, S, parts, rot, lut)
    assert_estimate(got, want)
    assert_estimate(run_estimate(M, S, parts, rot, lut), want)                      # two runs, equal bits
    m = M.moments(got[2].cpu().tolist())
    assert m == R.moments(want[2]) and m["W"] == int(want[1][-1]) and (n == 1 or 0 < m["positive"] < m["standing"] < n)


def test_estimate_at_the_contracts_extremes(built_lib):
    """65536 particles of weight 2^20 at x = y = 1 023 999: the sums of section 38's bound, none wraps."""
    from go_slam_amd import mcl as M
    N, x = 65536, 1023999
    parts = np.tile(np.array([[x, x, 0]], np.int32), (N, 1))
    w, cum, stats = run_estimate(M, np.zeros(N, np.uint32), parts, M.heading_table(1), np.array([1 << 20], np.uint32))
    W = N << 20
    assert bool((w == 1 << 20).all()) and torch.equal(cum.cpu(), torch.arange(1, N + 1, dtype=torch.int64) << 20)
    assert M.moments(stats.cpu().tolist()) == {"W": W, "W2": N << 40, "standing": N, "positive": N, "best": 0, "x": W * x,
                                               "y": W * x, "c": W << 14, "s": 0, "xx": W * x * x, "yy": W * x * x, "xy": W * x * x}
    assert stats[15].item() == 0 and all(0 <= v < 1 << 57 for v in stats.cpu().tolist())


def test_none_one_and_all_equal(built_lib):
    """No particle stands: best all ones, W 0, nothing to resample.  One stands: it is the best and has all the weight.
    Equal scores everywhere: best takes the lowest index."""
    from go_slam_amd import mcl as M
    rot, lut = M.heading_table(4), M.weight_table(60)
    blocked = np.full((5, 6), 100, dtype=np.uint8)
    parts = particles_on("scene", 257, 4) % np.array([5000, 6000, 4], dtype=np.int32)
    ends = ends_for("scene", 4, 64)
    for cells, allow in ((blocked, False), (blocked, True), (np.full((5, 6), 205, np.uint8), False)):
        cost = SR.field(cells, 3)
        S, best = M.weigh(gpu(cost), gpu(cells), gpu(parts), ends, 10, allow)
        assert bool((S == -1).all()) and best.item() == -1
        w, cum, stats = run_estimate(M, S, parts, rot, lut)
        assert not bool(w.any()) and not bool(cum.any())
        assert [v & MASK64 for v in stats.cpu().tolist()] == [0, 0, 0, 0, R.NO_BEST] + [0] * 11
    one = np.array(blocked)
    cell = (int(parts[200, 0]) // 1000, int(parts[200, 1]) // 1000)
    one[cell] = 254
    here = [p for p in range(257) if (int(parts[p, 0]) // 1000, int(parts[p, 1]) // 1000) == cell]
    keep = np.array(parts)
    keep[[p for p in here if p != 200], 0] = (cell[0] + 1) % 5 * 1000                # the others leave the one free cell
    cost = SR.field(one, 3)
    want = R.weigh(cost, one, keep, ends, 10, False)
    S, best = M.weigh(gpu(cost), gpu(one), gpu(keep), ends, 10, False)
    assert torch.equal(S.cpu(), torch.from_numpy(want[0].view(np.int32))) and best.item() & MASK64 == want[1]
    assert int((S != -1).sum()) == 1 and best.item() & 0xffffffff == 200
    w, cum, stats = run_estimate(M, S, keep, rot, lut)
    assert_estimate((w, cum, stats), R.estimate(want[0], keep, rot, lut))
    assert int(w[200]) == 1 << 20 and int(w.sum()) == 1 << 20 and stats[2].item() == 1
    got = M.resample(cum, gpu(keep), 1 << 20, (1 << 20) - 1)
    assert torch.equal(got.cpu(), torch.from_numpy(np.tile(keep[200], (257, 1))))
    free = np.full((5, 6), 254, dtype=np.uint8)                                      # no site: every end point costs the cap
    S, best = M.weigh(gpu(SR.field(free, 3)), gpu(free), gpu(parts), ends, 10, False)
    assert bool((S == 64 * 10).all()) and best.item() == (640 << 32)                # the lowest index wins the tie
    w, cum, stats = run_estimate(M, S, parts, rot, lut)
    assert bool((w == 1 << 20).all()) and stats[4].item() == 640 << 32 and stats[0].item() == 257 << 20


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1025, 4099])
def test_resample_equals_the_restatement(built_lib, n):
    from go_slam_amd import mcl as M
    rng = np.random.default_rng(n)
    parts = particles_on("scene", n, 360)
    weights = {"drawn": np.where(rng.random(n) < 0.3, 0, rng.integers(1, 1 << 20, n)), "first": np.eye(1, n, 0)[0] * 977,
               "last": np.eye(1, n, n - 1)[0] * (1 << 20), "middle": np.eye(1, n, n // 2)[0] * 3,
               "full": np.full(n, 1 << 20)}
    weights["drawn"][n // 2] = 1 << 20
    for key, w in weights.items():
        cum = np.cumsum(w.astype(np.int64)).astype(np.uint64)
        W = int(cum[-1])
        for q in (0, W - 1, W // 3):
            want = R.resample(cum, parts, W, q)
            out = torch.full((n, 3), -9, dtype=torch.int32, device=DEV)
            got = M.resample(cum, gpu(parts), W, q, out=out)
            assert got is out and torch.equal(out.cpu(), torch.from_numpy(want)), (key, q)
        if key in ("first", "last", "middle"):
            at = {"first": 0, "last": n - 1, "middle": n // 2}[key]
            assert torch.equal(out.cpu(), torch.from_numpy(np.tile(parts[at], (n, 1))))


def test_a_whole_tick_equals_the_restatement_twice(built_lib):
    """move, weigh, estimate and resample chained on the device as `ParticleFilter.tick` chains them, against
    mcl_restatement.tick with the same noise and the same draw; a second run gives the same bits."""
    from go_slam_amd import mcl as M
    cells, cost, rot, lut = MC.loop_tables()
    n = 1025
    rng = np.random.default_rng(8)
    start = np.rint(np.array(MC.LOOP_START) + rng.standard_normal((n, 3)) * np.array(MC.LOOP_SEED_SIGMAS)).astype(np.int64)
    start[:, 2] %= MC.LOOP_H
    start = start.astype(np.int32)
    noise = np.rint(rng.standard_normal((n, 3)) * np.array(MC.LOOP_SIGMAS)).astype(np.int32)
    ends = MC.loop_ends(0)
    want, info = R.tick(start, MC.LOOP_ROUTE[0], noise, ends, cost, cells, rot, lut, MC.LOOP_R ** 2 + 1, False, lambda: 0x9e3779b9)
    assert info["resampled"]
    runs = []
    for _ in range(2):
        p = M.move(gpu(start), rot, noise, MC.LOOP_ROUTE[0], cells.shape)
        S, best = M.weigh(gpu(cost), gpu(cells), p, ends, MC.LOOP_R ** 2 + 1)
        w, cum, stats = M.estimate(S, p, rot, lut)
        words = [v & MASK64 for v in stats.cpu().tolist()]
        assert words == info["stats"] and best.item() & MASK64 == info["best"] == words[4]
        runs.append((M.resample(cum, p, words[0], (0x9e3779b9 * words[0]) >> 32), S, w, cum))
        assert torch.equal(runs[-1][0].cpu(), torch.from_numpy(want))
    assert all(torch.equal(a, b) for a, b in zip(*runs))


# ---- refusals -----------------------------------------------------------------------------------------------------------
def test_c_abi_refusals_leave_the_outputs_untouched(built_lib):
    from go_slam_amd import _lib
    L, P = _lib.lib(), _lib.ptr
    stream = _lib.stream_ptr(DEV)
    n = 6
    parts = torch.tensor([[500, 500, 0], [1500, 2500, 1], [2500, 500, 2], [500, 4500, 3], [2999, 4999, 0], [0, 0, 1]],
                         dtype=torch.int32, device=DEV)
    rot = torch.tensor([[16384, 0], [0, 16384], [-16384, 0], [0, -16384]], dtype=torch.int32, device=DEV)
    noise = torch.zeros((n, 3), dtype=torch.int32, device=DEV)
    moved = torch.full((n, 3), -7, dtype=torch.int32, device=DEV)
    big = torch.full((2 * n, 3), -7, dtype=torch.int32, device=DEV)
    good = dict(particles=P(parts), n=n, rot=P(rot), n_headings=4, noise=P(noise), df=100, dl=0, dh=1, n_u=3, n_v=5, out=P(moved))
    step = (1 << 20) + 1
    bad = [("particles", None), ("rot", None), ("noise", None), ("out", None), ("n", -1), ("n", 65537), ("n_headings", 0),
           ("n_headings", 1025), ("df", step), ("df", -step), ("dl", step), ("dl", -step), ("dh", step), ("dh", -step), ("n_u", 0),
           ("n_u", 1025), ("n_v", 0), ("n_v", 1025)]
    for key, value in bad:
        assert L.gs_mcl_move(*{**good, key: value}.values(), stream) == INVALID, (key, value)
    # an output that overlaps the input without being it: one row further on in the same buffer
    overlap = dict(good, particles=P(big), out=P(big[1:]))
    assert L.gs_mcl_move(*overlap.values(), stream) == INVALID
    assert b"mcl_move" in L.gs_last_error()
    cells = torch.full((3, 5), 254, dtype=torch.uint8, device=DEV)
    cost = torch.ones((3, 5), dtype=torch.uint8, device=DEV)
    ends = torch.zeros((4, 3, 2), dtype=torch.int32, device=DEV)
    S = torch.full((n,), 12345, dtype=torch.int32, device=DEV)
    best = torch.full((2,), 999, dtype=torch.int64, device=DEV)
    good2 = dict(cost=P(cost), cells=P(cells), n_u=3, n_v=5, particles=P(parts), n=n, ends=P(ends), n_headings=4, n_beams=3,
                 cap=5, allow_unknown=0, S=P(S), best=P(best))
    bad2 = [("cost", None), ("cells", None), ("particles", None), ("ends", None), ("S", None), ("best", None), ("n_u", 0),
            ("n_u", 1025), ("n_v", 0), ("n_v", 1025), ("n", -1), ("n", 65537), ("n_headings", 0), ("n_headings", 1025),
            ("n_beams", 0), ("n_beams", 4097), ("cap", 0), ("cap", 227), ("allow_unknown", 2), ("allow_unknown", -1),
            ("ends", P(ends.view(-1)[1:])), ("best", P(best.view(torch.int32)[1:]))]
    for key, value in bad2:
        assert L.gs_mcl_weigh(*{**good2, key: value}.values(), stream) == INVALID, (key, value)
    assert b"mcl_weigh" in L.gs_last_error()
    lut = torch.tensor([1 << 20, 1000, 1], dtype=torch.int32, device=DEV)
    scores = torch.tensor([3, 4, -1, 3, 5, 9], dtype=torch.int32, device=DEV)
    w = torch.full((n,), -5, dtype=torch.int32, device=DEV)
    cum = torch.full((n + 1,), -5, dtype=torch.int64, device=DEV)
    stats = torch.full((17,), -5, dtype=torch.int64, device=DEV)
    good3 = dict(S=P(scores), particles=P(parts), n=n, rot=P(rot), n_headings=4, lut=P(lut), n_lut=3, w=P(w), cum=P(cum),
                 stats=P(stats))
    bad3 = [("S", None), ("particles", None), ("rot", None), ("lut", None), ("w", None), ("cum", None), ("stats", None),
            ("n", -1), ("n", 65537), ("n_headings", 0), ("n_headings", 1025), ("n_lut", 0), ("n_lut", 65537),
            ("cum", P(cum.view(torch.int32)[1:])), ("stats", P(stats.view(torch.int32)[1:]))]
    for key, value in bad3:
        assert L.gs_mcl_estimate(*{**good3, key: value}.values(), stream) == INVALID, (key, value)
    assert b"mcl_estimate" in L.gs_last_error()
    sums = torch.tensor([5, 5, 9, 9, 9, 10], dtype=torch.int64, device=DEV)
    fresh = torch.full((n, 3), -3, dtype=torch.int32, device=DEV)
    good4 = dict(cum=P(sums), particles=P(parts), n=n, W=10, q=3, out=P(fresh))
    bad4 = [("cum", None), ("particles", None), ("out", None), ("n", -1), ("n", 65537), ("W", 0), ("W", (1 << 36) + 1), ("q", 10),
            ("q", 1 << 40), ("out", P(parts)), ("cum", P(sums.view(torch.int32)[1:]))]
    for key, value in bad4:
        assert L.gs_mcl_resample(*{**good4, key: value}.values(), stream) == INVALID, (key, value)
    assert L.gs_mcl_resample(*dict(good4, particles=P(big), out=P(big[n - 1:])).values(), stream) == INVALID    # one shared row
    assert b"mcl_resample" in L.gs_last_error()
    torch.cuda.synchronize()
    assert bool((moved == -7).all()) and bool((big == -7).all()) and bool((S == 12345).all()) and bool((best == 999).all())
    assert bool((w == -5).all()) and bool((cum == -5).all()) and bool((stats == -5).all()) and bool((fresh == -3).all())
    # N == 0 launches nothing and writes nothing but the reset of best
    for call, args in ((L.gs_mcl_move, good), (L.gs_mcl_weigh, good2), (L.gs_mcl_estimate, good3), (L.gs_mcl_resample, good4)):
        assert call(*dict(args, n=0).values(), stream) == 0
    torch.cuda.synchronize()
    assert bool((moved == -7).all()) and bool((S == 12345).all()) and best.tolist() == [-1, 999] and bool((stats == -5).all())
    assert bool((fresh == -3).all())
    assert L.gs_mcl_move(*good.values(), stream) == 0 and L.gs_mcl_weigh(*good2.values(), stream) == 0
    assert L.gs_mcl_estimate(*good3.values(), stream) == 0 and L.gs_mcl_resample(*good4.values(), stream) == 0
    torch.cuda.synchronize()
    assert moved.tolist() == [[600, 500, 1], [1500, 2600, 2], [2400, 500, 3], [500, 4400, 0], [2999, 4999, 1], [0, 100, 2]]
    assert S.tolist() == [3] * n and best.tolist() == [3 << 32, 999]
    assert w.tolist() == [1 << 20, 1000, 0, 1 << 20, 1, 0] and cum[n].item() == -5 and stats[16].item() == -5
    assert cum[:n].tolist() == np.cumsum(w.tolist()).tolist() and stats[:5].tolist() == [cum[n - 1].item(), (1 << 41) + 1000001, 5, 4, 3 << 32]
    # thresholds (10 j + 3) against cum * 6 = 30, 30, 54, 54, 54, 60
    assert fresh.tolist() == [parts[i].tolist() for i in (0, 0, 0, 2, 2, 2)]


def test_wrappers_refuse_aliasing(built_lib):
    from go_slam_amd import mcl as M
    buf = torch.zeros((10, 3), dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="mcl.move"):
        M.move(buf[:6], M.heading_table(4), np.zeros((6, 3), np.int32), (0, 0, 0), (3, 5), out=buf[2:8])
    with pytest.raises(ValueError, match="mcl.resample"):
        M.resample(np.arange(1, 7, dtype=np.uint64), buf[:6], 6, 0, out=buf[:6])
    with pytest.raises(ValueError, match="mcl.resample"):
        M.resample(np.arange(1, 7, dtype=np.uint64), buf[:6], 6, 0, out=buf[4:10])
    with pytest.raises(ValueError, match="ParticleFilter.tick"):
        M.ParticleFilter(SC.scene_grid(), 64, 36, n_beams=60).tick((0, 0, 0), [1.0], [0.0], (1, 1, 1))


# ---- the closed loop ----------------------------------------------------------------------------------------------------
def loop_filter(M, seed, **kw):
    grid = {"cells": gpu(SC.scene()), "origin": (0.0, 0.0), "resolution": 1.0}
    pf = M.ParticleFilter(grid, MC.LOOP_N, MC.LOOP_H, n_beams=MC.LOOP_BEAMS, radius_cells=MC.LOOP_R, seed=seed,
                          max_range=float(MC.LOOP_RANGE), **kw)
    x, y, h = MC.LOOP_START
    pf.seed_around((x / 1000.0, y / 1000.0), 2.0 * math.pi * h / MC.LOOP_H, MC.LOOP_SEED_SIGMAS[0] / 1000.0,
                   MC.LOOP_SEED_SIGMAS[2] * 2.0 * math.pi / MC.LOOP_H)
    return pf


def loop_errors(est, true):
    return (math.hypot(est["milli"][0] - true[0], est["milli"][1] - true[1]) / 1000.0, MC.heading_apart(est["heading"], true[2]))


@pytest.mark.parametrize("seed", MC.LOOP_SEEDS)
def test_particle_filter_tracks_the_closed_loop(built_lib, seed):
    """The route of tests/test_mcl_cpu.py with the filter's own noise (the device generator's: another sample of the same
    loop): the worst error stays within 1.5 times the restatement's recorded worst and below a third of the 3.05 cells of
    the reported odometry alone; `lost` is never raised."""
    from go_slam_amd import mcl as M
    pf = loop_filter(M, seed)
    start = pf.particles.cpu().numpy()
    assert abs(float(start[:, 0].mean()) - MC.LOOP_START[0]) < 200 and 800 < float(start[:, 0].std()) < 1200
    worst, turn, resampled = 0.0, 0.0, 0
    for t, (step, true, (ranges, angles)) in enumerate(zip(MC.LOOP_ROUTE, MC.loop_truth(), MC.loop_scans())):
        est = pf.tick(MC.reported(t, step), ranges, angles, MC.LOOP_SIGMAS)
        assert est["found"] and not est["lost"] and not pf.lost and est["n_standing"] > 0, t
        assert est["n_beams"] == int(np.isfinite(ranges).sum()) and 0.0 < est["ess"] <= MC.LOOP_N
        assert est["cell"] == (int(est["milli"][0]) // 1000, int(est["milli"][1]) // 1000)
        assert est["xy"] == (est["milli"][0] / 1000.0, est["milli"][1] / 1000.0) and 0.0 < est["yaw_concentration"] <= 1.0
        assert est["cov"][0][0] >= 0.0 and est["cov"][1][1] >= 0.0 and est["cov"][0][1] == est["cov"][1][0]
        e, a = loop_errors(est, true)
        worst, turn, resampled = max(worst, e), max(turn, a), resampled + est["resampled"]
    print(f"seed {seed}: worst position error {worst:.4f} cells (restatement {MC.LOOP_RECORDED[seed][0]}), worst heading "
          f"error {turn:.3f} steps, resampled {resampled} of {len(MC.LOOP_ROUTE)} ticks")
    assert worst <= 1.5 * MC.LOOP_RECORDED[seed][0] and worst < MC.LOOP_DEAD_RECKONED_CELLS / 3.0
    assert turn <= 5.0 and resampled > 0


def test_a_kidnapped_filter_reports_lost_and_recovers(built_lib):
    """Before tick 20 the particles are put around (40500, 30500) and turned by 120 steps: `lost` rises within lost_ticks
    ticks, `recover` finds the pose again by the exhaustive match, and the next tick is within 1.5 cells."""
    from go_slam_amd import mcl as M
    pf = loop_filter(M, 0)
    assert pf.lost_ticks == 3
    lost_at, errors = None, {}
    for t, (step, true, (ranges, angles)) in enumerate(zip(MC.LOOP_ROUTE, MC.loop_truth(), MC.loop_scans())):
        if t == 20:
            h = MC.loop_truth()[19][2] + 120
            pf.seed_around((40.5, 30.5), 2.0 * math.pi * h / MC.LOOP_H, 1.0, 3 * 2.0 * math.pi / MC.LOOP_H)
        est = pf.tick(MC.reported(t, step), ranges, angles, MC.LOOP_SIGMAS)
        if est["found"]:
            errors[t] = loop_errors(est, true)[0]
        if t < 20:
            assert not est["lost"]
        if est["lost"] and lost_at is None:
            lost_at = t
            found = pf.recover(ranges, angles)
            print(f"lost at tick {t} (best mean cost {est['best_mean_cost']}, standing {est['n_standing']}); recovered", found)
            assert found["found"] and not pf.lost
            assert max(abs(found["cell"][0] - true[0] // 1000), abs(found["cell"][1] - true[1] // 1000)) <= 1
        elif lost_at is not None:
            assert not est["lost"], t
        if t == 23:
            break
    assert lost_at is not None and 20 <= lost_at < 20 + pf.lost_ticks
    assert errors.get(20, 99.0) > 5.0 and errors[lost_at + 1] < 1.5
    print("errors in cells by tick:", {t: round(e, 3) for t, e in errors.items() if t >= 18})


def test_seed_free_and_step_in_metres(built_lib):
    from go_slam_amd import mcl as M
    cells = SC.scene()
    grid = {"cells": gpu(cells), "origin": (-1.0, 2.0), "resolution": 0.05}
    pf = M.ParticleFilter(grid, 4099, 90, n_beams=MC.LOOP_BEAMS, seed=3, max_range=MC.LOOP_RANGE * 0.05)
    pf.seed_free()
    p = pf.particles.cpu().numpy()
    assert (cells[p[:, 0] // 1000, p[:, 1] // 1000] == 254).all() and 0 <= p[:, 2].min() and p[:, 2].max() < 90
    assert len(np.unique(p[:, 2])) > 60 and len(np.unique(p[:, 0] // 1000)) > 30
    pf.seed_around((-1.0 + 10.5 * 0.05, 2.0 + 10.5 * 0.05), 0.0, 0.05, 0.05)
    ranges, angles = MC.loop_scans()[0]
    est = pf.step((0.05, 0.0, 0.0), ranges * 0.05, angles)        # one cell forward: the first tick of the route
    true = MC.loop_truth()[0]
    assert est["found"] and not est["lost"] and est["n_standing"] > 3000
    assert math.hypot(est["xy"][0] - (-1.0 + true[0] / 1000.0 * 0.05), est["xy"][1] - (2.0 + true[1] / 1000.0 * 0.05)) < 0.05
    assert abs(est["yaw"]) < 0.1 and est["cov"][0][0] < 0.05 ** 2 * 4


# ---- one config-driven run ----------------------------------------------------------------------------------------------
def test_only_tracking_run_ends_with_the_mcl_file(built_lib, tmp_path, monkeypatch):
    from go_slam_amd import mcl as M
    from go_slam_amd import scan as S
    from go_slam_amd.slam import SLAM
    returned = []
    terminate = SLAM.terminate

    def keeping(self, *args, **kw):
        returned.append(terminate(self, *args, **kw))
        return returned[-1]
    monkeypatch.setattr(SLAM, "terminate", keeping)
    out = str(tmp_path / "with")
    # the slab of tests/test_scan_gpu.py's run: up along z, just in front of the wall at z = 4
    slab = {"up_axis": 2, "height": [3.0, 3.6], "beams": 48, "fov_deg": 270.0, "max_range": 3.0}
    scan_cfg = dict(slab, every=2, n_yaw=24, window_m=0.5)
    mcl_cfg = dict(slab, every=1, particles=256, headings=72, drift={"scale": 1.02, "yaw_deg_per_m": 1.0}, seed=1)
    cfg = {"enable": True, "source": "sensor", "voxel_size": 0.1,
           "esdf": {"enable": True, "max_distance": 1.0, "scan": scan_cfg, "mcl": mcl_cfg}}
    EG.TG.whole_run(out, cfg)
    stats = returned[0]
    text = open(f"{out}/map/mcl.txt").read()
    report = M.parse_mcl(text)
    print("map/mcl.txt:", {k: report[k] for k in M.MCL_SUMMARY_ORDER}, report["rows"][:2])
    assert M.mcl_text(report) == text
    n_poses = len(np.load(f"{out}/checkpoints/est_poses.npy"))
    assert report["particles"] == 256 and report["headings"] == 72 and report["ticks"] == len(report["rows"]) >= 1
    assert report["ticks"] + report["poses_skipped"] + 1 == n_poses                  # the first pose used seeds the filter
    assert report["relocalized"] == sum(r["relocalized"] for r in report["rows"])
    assert report["max_error_m"] == max(r["error_m"] for r in report["rows"])
    assert any(r["n_standing"] > 0 and math.isfinite(r["error_m"]) for r in report["rows"])
    assert stats["tsdf_mcl_ticks"] == report["ticks"] and stats["tsdf_mcl_max_error_m"] == report["max_error_m"]
    assert stats["tsdf_mcl_relocalized"] == report["relocalized"]
    assert os.path.exists(f"{out}/map/scan_localize.txt") and S.parse_scan_localize(open(f"{out}/map/scan_localize.txt").read())
    listing = EG.TG.listing(out)
    assert os.path.join("map", "mcl.txt") in listing and os.path.join("map", "scan_localize.txt") in listing
