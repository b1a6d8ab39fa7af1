"""What the cost field and the frontier labels share, the brick sweep of csrc/brick_relax.h, on the MI355X: a brick whose
rounds inside LDS run out marks itself and goes on in the next sweep, and the sweeps, their `changed` words and the fixed
point do not depend on how many sweeps one C call enqueues."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import frontier_restatement as FR                              # noqa: E402
import geodesic_restatement as GR                              # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROUNDS_MAX = 64                                                # GEO_ROUNDS_MAX, FRONTIER_ROUNDS_MAX


def corridor(brick):
    """bool [b0, b1, 2 * b2]: a one-cell-wide serpentine inside the first of the two bricks -- a row along the last axis
    at every even (x, y), walked boustrophedon, consecutive rows joined by one cell at the end they share -- and nothing
    in the second brick.  Rows are two cells apart, so only the joints connect them, under 26-connectivity too."""
    b0, b1, b2 = brick
    path = np.zeros((b0, b1, 2 * b2), dtype=bool)
    rows = [(x, y) for i, x in enumerate(range(0, b0, 2)) for y in list(range(0, b1, 2))[::1 if i % 2 == 0 else -1]]
    for n, (x, y) in enumerate(rows):
        path[x, y, :b2] = True
        if n + 1 < len(rows):
            nx, ny = rows[n + 1]
            path[(x + nx) // 2, (y + ny) // 2, b2 - 1 if n % 2 == 0 else 0] = True
    return path


@pytest.mark.parametrize("which", ["geodesic", "frontier"])
def test_a_brick_that_runs_out_of_rounds_marks_itself(built_lib, which):
    """One brick by two along the last axis, a corridor of more than ROUNDS_MAX cells in the first brick, nothing in the
    second: the second brick never lowers a cell, so the first is marked again by nobody but itself, and the fixed
    point of the restatement is only reached if it does so when its rounds run out."""
    from go_slam_amd import frontier, plan
    brick = plan.brick() if which == "geodesic" else frontier.brick()
    path = corridor(brick)
    inside = int(path[:, :, :brick[2]].sum())
    print("brick", brick, "corridor cells", inside)
    assert inside > ROUNDS_MAX and not path[:, :, brick[2]:].any()
    if which == "geodesic":
        ref = GR.field(path, [(0, 0, 0)])
        assert int((ref < GR.INF).sum()) == inside and ref[path].max() == 1000 * (inside - 1)      # connected, one wide
        field = plan.geodesic_field(torch.from_numpy(path).to(DEV), [(0, 0, 0)])
        print("sweeps", field.sweeps)
        assert torch.equal(field.cost.cpu(), torch.from_numpy(ref))
        assert field.sweeps >= 2
    else:
        state = np.where(path, 1, 0).astype(np.uint8)          # free on the corridor, unknown beside it
        state[:, :, brick[2]:] = 2
        ref = FR.clusters(state)
        assert np.array_equal(ref["frontier"] != 0, path)
        assert len(ref["root"]) == 1 and ref["root"][0] == 0 and ref["size"][0] == inside      # connected
        fc = frontier.frontier_clusters(torch.from_numpy(state).to(DEV))
        print("sweeps", fc.sweeps)
        assert torch.equal(fc.label.cpu(), torch.from_numpy(ref["label"]))
        assert fc.n_clusters == 1 and int(fc.size[0]) == inside
        assert fc.sweeps >= 2


def drive(which, state, k):
    """The field or the labels of `state` through the C ABI with k sweeps per call, one read of changed[:k] per call:
    (result on the host, every changed word read, in order)."""
    from go_slam_amd import _lib
    L, P = _lib.lib(), _lib.ptr
    stream = _lib.stream_ptr(DEV)
    dims = state.shape
    changed = torch.full((k,), 7, dtype=torch.int32, device=DEV)
    out = torch.empty(dims, dtype=torch.int32, device=DEV)
    if which == "geodesic":
        passable = torch.from_numpy((state != 2).astype(np.uint8)).to(DEV)
        free = np.argwhere(state != 2)
        seed = torch.tensor(free[len(free) // 2:len(free) // 2 + 1], dtype=torch.int32, device=DEV)      # mid-lattice
        flags = torch.empty(L.gs_geodesic_flags_bytes(*dims), dtype=torch.uint8, device=DEV)
        assert L.gs_geodesic_init(P(passable), *dims, P(seed), 1, P(out), P(flags), stream) == 0

        def relax(sweep0):
            return L.gs_geodesic_relax(P(passable), *dims, GR.MAX_COST, P(out), P(flags), sweep0, k, P(changed), stream)
    else:
        cells = torch.from_numpy(state).to(DEV)
        fr = torch.empty(dims, dtype=torch.uint8, device=DEV)
        counts = torch.empty(4, dtype=torch.int32, device=DEV)
        flags = torch.empty(L.gs_frontier_flags_bytes(*dims), dtype=torch.uint8, device=DEV)
        assert L.gs_frontier_mark(P(cells), None, *dims, P(fr), P(out), P(counts), P(flags), stream) == 0

        def relax(sweep0):
            return L.gs_frontier_relax(*dims, P(out), P(flags), sweep0, k, P(changed), stream)
    words = []
    while 0 not in words:
        assert len(words) < 4096
        assert relax(len(words)) == 0
        words += changed.cpu().tolist()
    return out.cpu(), words


@pytest.mark.parametrize("which", ["geodesic", "frontier"])
def test_one_sweep_per_call_and_a_batch_per_call_agree(built_lib, which):
    from go_slam_amd import frontier, plan
    assert frontier.SWEEP_BATCH == plan.SWEEP_BATCH > 1
    state = np.random.default_rng(12).integers(0, 3, size=(9, 10, 70)).astype(np.uint8)
    one, words_one = drive(which, state, 1)
    batch, words_batch = drive(which, state, plan.SWEEP_BATCH)
    sweeps = words_one.index(0) + 1
    print(which, "sweeps", sweeps, "batched", words_batch.index(0) + 1)
    assert sweeps >= 3 and int((one != (GR.INF if which == "geodesic" else -1)).sum()) > state.size // 4      # not vacuous
    assert set(words_one) <= {0, 1} and set(words_batch) <= {0, 1}
    assert words_one == [1] * (sweeps - 1) + [0]
    assert words_batch[:sweeps] == words_one and not any(words_batch[sweeps:])      # sweeps past the fixed point do nothing
    assert torch.equal(one, batch)
