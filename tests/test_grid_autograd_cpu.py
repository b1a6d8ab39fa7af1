"""Pins tests/grid_autograd_restatement.py (the fp64 restatement of gs_grid_encode and gs_grid_backward) without a GPU:
its values per element against oracle/neus_autograd.py's grid_encode_diff in float64 (the encoding and dy_dx directly,
the first order by torch.autograd.grad, the second order by double backward through x_differentiable=True), per level
slice of the table and per one-hot level of the upstream gradient; its bounds against vacuity by
test_neus_bwd_cpu._vacuity; its deliberately wrong variants against the bounds, which each must leave; the fp16 table's
overflow flag on the scene / upstream pairs tests/test_grid_autograd_numerics_gpu.py runs; and grid_corners' modulo branch
(x = 1 on the dense levels) against the oracle's index.

The autograd oracle builds a 12.6 M-entry table gradient per call, so one evaluation serves all scenes: the scenes are
concatenated into one batch (per-point outputs are compared per scene section, the table on the whole batch), and a
level's table slice and a level's share of dx follow from linearity in dy: the table gradient of level l depends on dy's
two level-l features alone and lands in level l's slice alone, and the per-level dx comes from autograd.grad of that
level's term with respect to x (which never visits the table)."""
import numpy as np
import pytest
import torch

import grid_autograd_restatement as G
import neus_bwd_restatement as R
from oracle import neus_autograd as NA
from oracle import neus_oracle as NO
from test_neus_bwd_cpu import _vacuity

SECTIONS = (("uniform", 130), ("clump", 257), ("ray", 257), ("faces", 65), ("corners", 65), ("one", 1))
LV = range(NO.N_LEVELS)


@pytest.fixture(scope="module")
def meta():
    return NO.grid_meta()


@pytest.fixture(scope="module")
def batch(meta):
    xs = [G.scene(s, n, seed=11 + i, meta=meta) for i, (s, n) in enumerate(SECTIONS)]
    edges = np.cumsum([0] + [len(x) for x in xs])
    x = np.concatenate(xs)
    dy, v = G.upstream(len(x), 3)
    return dict(x=x, dy=dy, v=v, sections=[(s, int(a), int(b)) for (s, _), a, b in zip(SECTIONS, edges, edges[1:])])


def _oracle(x, grid16, dy, v, meta, table=True):
    """float64 autograd on grid_encode_diff: enc, dydx; first order dx1 (+ per level), gg1; second order ddy, dx2 (+ per
    level), gg2"""
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        t = lambda a, rg=False: torch.tensor(np.asarray(a, np.float64), requires_grad=rg)
        xt, g, dyt, vt = t(x, True), t(grid16, True), t(dy, True), t(v)
        enc, dydx = NA.grid_encode_diff(xt, g, meta, x_differentiable=True)
        grad = lambda L, ins: [a.numpy() for a in torch.autograd.grad(L, ins, retain_graph=True)]
        term1 = lambda sl: (enc[:, sl] * dyt[:, sl]).sum()
        term2 = lambda sl: (torch.einsum("ncd,nc->nd", dydx[:, sl], dyt[:, sl]) * vt).sum()
        full = slice(0, 32)
        out = dict(enc=enc.detach().numpy(), dydx=dydx.detach().numpy())
        if table:
            out["dx1"], out["gg1"] = grad(term1(full), [xt, g])
            out["ddy"], out["dx2"], out["gg2"] = grad(term2(full), [dyt, xt, g])
            out["dx1_l"] = [grad(term1(slice(2 * l, 2 * l + 2)), [xt])[0] for l in LV]
            out["dx2_l"] = [grad(term2(slice(2 * l, 2 * l + 2)), [xt])[0] for l in LV]
        else:
            out["dx1"], = grad(term1(full), [xt])
            out["ddy"], out["dx2"] = grad(term2(full), [dyt, xt])
        return out
    finally:
        torch.set_default_dtype(old)


@pytest.fixture(scope="module")
def flat_grid(meta):
    return G.table("flat", 0, meta)


@pytest.fixture(scope="module")
def flat(meta, batch, flat_grid):
    grid = flat_grid
    return grid, _oracle(batch["x"], grid, batch["dy"], batch["v"], meta)


@pytest.fixture(scope="module")
def init(meta, batch):
    # (the table gradient does not depend on the table's values: the flat table's evaluation pins it)
    grid = G.table("init", 1, meta)
    return grid, _oracle(batch["x"], grid, batch["dy"], batch["v"], meta, table=False)


def _pin(got, ref, what, slack=1e-2):
    """the restated value is the oracle's: within 1e-9 relative (the oracle's own float64 arithmetic) plus a hundredth
    of the bound (both evaluate the same formula, so the bound itself is never needed)"""
    ref = np.asarray(ref, np.float64)
    err = np.abs(got.v - ref)
    tol = 1e-9 * np.abs(ref) + slack * got.e + 1e-300
    bad = ~(err <= tol)
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {err.size} off the oracle, first {np.argwhere(bad)[0].tolist()}: "
                           f"{got.v[bad][0]} vs {ref[bad][0]} (bound {got.e[bad][0]})")


def _pin_table(tab, gg, meta, what, levels=LV):
    """per level slice: the restated entries against autograd's, and no entry reached by one and not the other; the
    slices of the levels not in `levels` (one-hot upstreams) hold nothing"""
    idx = tab["idx"]
    for l in LV:
        a, b = G.level_slice(meta, l)
        lo, hi = np.searchsorted(idx, [a, b])
        if l in levels:
            at = idx[lo:hi]
            _pin(R.E(tab["value"][lo:hi], tab["bound"][lo:hi]), gg[at], f"{what}: table, level {l}")
            assert np.count_nonzero(gg[a:b]) == np.count_nonzero(gg[at]), \
                f"{what}: autograd reaches an entry of level {l} the restatement does not"
        else:
            assert lo == hi, f"{what}: level {l}'s slice is reached"


MODES = [("f32", 1.0), ("f32", 128.0), ("f16", 128.0)]


@pytest.fixture(scope="module")
def restated(meta, batch, flat, init):
    """the restatement on the whole batch, once per table: encode, first order, second order (every table mode)"""
    out = {}
    for kind, (grid, _) in (("flat", flat), ("init", init)):
        modes = MODES if kind == "flat" else MODES[:1]      # (the table gradient does not depend on the table's values)
        out[kind] = dict(enc=G.encode(batch["x"], grid, meta),
                         first=G.backward(batch["x"], grid, batch["dy"], tables=modes, meta=meta),
                         second=G.backward(batch["x"], grid, batch["dy"], v=batch["v"], tables=modes, meta=meta))
    return out


@pytest.mark.parametrize("kind", ["flat", "init"])
def test_encode_matches_the_oracle(kind, batch, flat, init, restated):
    ref = (flat if kind == "flat" else init)[1]
    got = restated[kind]["enc"]
    for s, a, b in batch["sections"]:
        _pin(got["out"][a:b], ref["enc"][a:b], f"{kind} {s}: out", slack=1.0)        # (the oracle's enc is fp16-rounded)
        _pin(got["dy_dx"][a:b], ref["dydx"][a:b], f"{kind} {s}: dy_dx")


@pytest.mark.parametrize("kind", ["flat", "init"])
def test_first_order_matches_autograd(kind, meta, batch, flat, init, restated):
    ref = (flat if kind == "flat" else init)[1]
    got = restated[kind]["first"]
    for s, a, b in batch["sections"]:
        _pin(got["dx"][a:b], ref["dx1"][a:b], f"{kind} {s}: dx")
    if kind == "flat":
        _pin_table(got["table"], ref["gg1"], meta, kind)
    assert "ddy" not in got


@pytest.mark.parametrize("kind", ["flat", "init"])
def test_second_order_matches_double_backward(kind, meta, batch, flat, init, restated):
    ref = (flat if kind == "flat" else init)[1]
    got = restated[kind]["second"]
    for s, a, b in batch["sections"]:
        _pin(got["ddy"][a:b], ref["ddy"][a:b], f"{kind} {s}: ddy")
        _pin(got["dx"][a:b], ref["dx2"][a:b], f"{kind} {s}: dx")
    if kind == "flat":
        _pin_table(got["table"], ref["gg2"], meta, kind)


def test_one_hot_levels_match_autograd(meta, batch, flat):
    """dy with only level l's two features non-zero, for every l: dx, ddy and the level's table slice alone"""
    grid, ref = flat
    x, v = batch["x"], batch["v"]
    for l in LV:
        dy, _ = G.upstream(len(x), 3, level=l)
        assert np.array_equal(dy[:, 2 * l:2 * l + 2], batch["dy"][:, 2 * l:2 * l + 2]) and np.count_nonzero(dy) <= 2 * len(x)
        one = G.backward(x, grid, dy, meta=meta)
        _pin(one["dx"], ref["dx1_l"][l], f"first order, level {l}: dx")
        _pin_table(one["table"], ref["gg1"], meta, f"first order, level {l}", levels=(l,))
        two = G.backward(x, grid, dy, v=v, meta=meta)
        _pin(two["dx"], ref["dx2_l"][l], f"second order, level {l}: dx")
        _pin(two["ddy"], ref["ddy"], f"second order, level {l}: ddy")
        _pin_table(two["table"], ref["gg2"], meta, f"second order, level {l}", levels=(l,))


@pytest.mark.parametrize("variant", ["f16_axis0", "scaled_axis1", "f16_scaled_axis2"])
def test_upstream_variants_match_autograd(variant, meta, batch, flat):
    """dy in fp16, dy_scale != 1 and v along one axis: dx and ddy against autograd on the upstream the kernel reads"""
    grid, _ = flat
    x = batch["x"][100:400]
    dt = "f16" if "f16" in variant else "f32"
    sc = 1.0 / 128 if "scaled" in variant else 1.0
    dy, v = G.upstream(len(x), 4, dt, sc, v=int(variant[-1]))
    ref = _oracle(x, grid, dy.astype(np.float64) * sc, v, meta, table=False)
    _pin(G.backward(x, grid, dy, sc, meta=meta)["dx"], ref["dx1"], f"{variant}: first-order dx")
    two = G.backward(x, grid, dy, sc, v=v, meta=meta)
    _pin(two["dx"], ref["dx2"], f"{variant}: second-order dx")
    _pin(two["ddy"], ref["ddy"], f"{variant}: ddy")


# ---------------------------------------------------------------------------------------------------- vacuity ----
@pytest.mark.parametrize("name", ["uniform", "clump", "ray"])
def test_bounds_are_not_vacuous(name, batch, restated):
    """per-point outputs on the scene's section of the batch, the table gradient on the whole batch"""
    r = restated["flat"]
    a, b = next((a, b) for s, a, b in batch["sections"] if s == name)
    V = lambda x: _vacuity(x.v[a:b], x.e[a:b])
    assert V(r["enc"]["out"]) < 1e-3, f"{name} out: {V(r['enc']['out'])}"
    assert V(r["enc"]["dy_dx"]) < 1e-4, f"{name} dy_dx: {V(r['enc']['dy_dx'])}"
    for order in ("first", "second"):
        got = r[order]
        for k in ("dx", "ddy"):
            if k in got:
                assert V(got[k]) < 1e-4, f"{name} {order} {k}: {V(got[k])}"
        for m, t in got["tables"].items():
            lim = 1e-4 if m[0] == "f32" else 1e-2
            assert _vacuity(t["value"], t["bound"]) < lim, f"{order} table {m}: {_vacuity(t['value'], t['bound'])}"
            assert not t["overflow"].any()


def test_bounds_of_the_initial_table(batch, restated):
    """tcnn's initial table U(-1e-4, 1e-4): the values are fp16 numbers of a few significant bits whose first and second
    corner differences cancel, so the bound relative to the value is what the cancellation leaves.  The limits are what
    the restatement alone reaches on the batch's uniform section (measured here on the CPU, rounded up to the next power
    of ten); they are not a tolerance of the kernel."""
    r = restated["init"]
    a, b = next((a, b) for s, a, b in batch["sections"] if s == "uniform")
    V = lambda x: _vacuity(x.v[a:b], x.e[a:b])
    seen = {"out": V(r["enc"]["out"]), "dy_dx": V(r["enc"]["dy_dx"]), "ddy": V(r["second"]["ddy"]),
            "dx": V(r["second"]["dx"]), "dx1": V(r["first"]["dx"])}
    print(seen)
    assert all(seen[k] < INIT_LIMITS[k] for k in INIT_LIMITS), seen


# measured: out 2.1e-2 (values of ~1e-5 against fp16's absolute 2^-25), dy_dx 3.5e-6, ddy 7.3e-6, dx 1.6e-5
INIT_LIMITS = {"out": 1e-1, "dy_dx": 1e-5, "ddy": 1e-5, "dx": 1e-4, "dx1": 1e-4}


# ---------------------------------------------------------------------------------------------------- mutants ----
def _table_breaks(right, wrong):
    idx = np.union1d(right["idx"], wrong["idx"])
    def on(t, key):
        a = np.zeros(idx.size)
        a[np.searchsorted(idx, t["idx"])] = t[key]
        return a
    return bool((np.abs(on(wrong, "value") - on(right, "value")) > on(right, "bound")).any())


_right = {}


@pytest.mark.parametrize("wrong", G.WRONG)
def test_wrong_variants_leave_the_bounds(wrong, meta, flat_grid):
    """every deliberately wrong variant leaves the bound of the output it touches, on a DENSE upstream: within the bounds
    no fine level covers a coarse one (the one-hot upstreams, where the level stands alone, are the GPU test's)"""
    grid = flat_grid
    x = G.scene("clump", 130, seed=8, meta=meta)
    mode = ("f16", 128.0) if wrong == "swap_features" else ("f32", 1.0)
    dy, v = G.upstream(len(x), 9)
    kw = dict(v=v, table_mode=mode[0], gg_scale=mode[1], meta=meta)
    if mode not in _right:
        _right[mode] = G.backward(x, grid, dy, **kw)
    right, bad = _right[mode], G.backward(x, grid, dy, _wrong=wrong, **kw)
    if wrong in ("s0_sign", "swap_features", "first_lane"):
        assert _table_breaks(right["table"], bad["table"]), f"{wrong}: the table stays within the bounds"
        assert np.array_equal(right["dx"].v, bad["dx"].v)
    else:
        assert (np.abs(bad["dx"].v - right["dx"].v) > right["dx"].e).any(), f"{wrong}: dx stays within the bounds"


# --------------------------------------------------------------------------------------------------- overflow ----
@pytest.mark.parametrize("name", G.SCENES)
def test_fp16_table_does_not_overflow_on_the_gpu_cases(name, meta):
    """the scene / upstream pairs of tests/test_grid_autograd_numerics_gpu.py: no entry of the fp16 table may overflow (so
    that file skips no entry; it asserts the same on every batch it runs, the larger ones included).  The upstream
    variants of one seed hold the same gradient: the fp16 and the scaled dy differ from the f32 one by a rounding, and a
    v along one axis is the dense v with two components zeroed, so its records are no larger -- the dense f32 and the
    scaled fp16 upstream stand for all six."""
    x = G.scene(name, 257, seed=1, meta=meta)
    for i in (0, 3):
        dt, sc, lv, vk = G.UPSTREAMS[i]
        dy, v = G.upstream(len(x), 2, dt, sc, level=lv, v="dense")
        for vv in (None, v):
            t = G.backward(x, None, dy, sc, v=vv, table_mode="f16", gg_scale=128.0, meta=meta)["table"]
            assert not t["overflow"].any(), f"{name} {dt} {sc} level {lv} v {vk}: {int(t['overflow'].sum())} entries"
            assert t["idx"].size > 0


# -------------------------------------------------------------------------------------------- grid_corners, x = 1 ----
def test_grid_corners_modulo_branch_matches_the_oracle(meta):
    """x = 1: the cell is resolution - 1 (scale + 0.5 floors to ceil(scale) = resolution - 1 ... or scale itself), its
    upper corners lie past a dense level's size, and `% size` runs"""
    dense = [l for l in LV if not int(meta["hashed"][l])]
    assert dense
    wrapped = 0
    for l in dense:
        x = np.array([[1, 1, 1], [1, 0.5, 0.25], [0.5, 1, 1], [0, 0, 1]], np.float32)
        gi, _ = R.cells(x, float(meta["scale"][l]))
        got = R.grid_corners(meta, l, gi)
        for c in range(8):
            corner = torch.tensor(gi.astype(np.int64) + [(c >> d) & 1 for d in range(3)])
            raw = corner[:, 0] + corner[:, 1] * int(meta["resolution"][l]) + corner[:, 2] * int(meta["resolution"][l]) ** 2
            wrapped += int((raw >= int(meta["size"][l])).sum())
            assert np.array_equal(got[:, c], NA._index(meta, l, corner).numpy()), f"level {l} corner {c}"
    assert wrapped > 0, "no corner index passed a dense level's size"
