"""The hash-grid encoding's generic autograd kernels -- gs_grid_encode with its dy_dx output (go_slam_amd/csrc/neus.hip) and
gs_grid_backward (go_slam_amd/csrc/grid_autograd.hip), everything the `tinycudann` drop-in gives the reference's code --
against the fp64 restatement in tests/grid_autograd_restatement.py, per element and per level.

Both kernels are called through the C ABI (ctypes).  Every output buffer is filled with a NaN sentinel first and has a
guard region behind it; the table gradient is zeroed but keeps a NaN guard.  Checked:
  shapes       n in {1, 63, 64, 65, 255, 256, 257, 4099} for every scene of the restatement (uniform, clump, ray, faces,
               corners, one), and 4096 x 72 points of the ray scene (what the drop-in sees from the mapper)
  tables       |grid| ~ 0.3, and tcnn's initial U(-1e-4, 1e-4)
  upstreams    dy in f32 and f16 with dy_scale 1 and 1/128; v dense and along one axis; one-hot-per-level dy at n = 4099
               (each level's dx, ddy and table slice alone; every other level's slice exactly 0)
  table modes  f32 (gg_scale 1 and 128) and f16 (gg_scale 128)
  outputs      every combination of requested outputs the launcher accepts -- first order: table, dx, both; second order:
               table, dx, ddy, all three (the drop-in sends: first order dx alone and table alone, second order whatever
               needs_input_grad asks, all three under the reference's use) -- an output passed as NULL leaves its buffer and
               every guard untouched
  assertions   out within one fp16 rounding of the restated fp32 value's interval; dy_dx, dx, ddy and every table entry
               within the restatement's bound; entries no record reaches exactly 0; nothing past n rows; out, dy_dx, dx,
               ddy bit-equal across two runs; dy_dx of gs_grid_encode bit-equal to the dv gs_grid_backward implies (ddy with
               v a unit vector, one axis at a time); the fp16 table's overflow flag empty on every batch
  refusals     ddy without v, dx without grid, a dy or table dtype that is neither GS_F16 nor GS_F32, n < 0: refused with
               nothing written; n == 0 a no-op
The worst error / bound ratio per output is written to $GRID_AUTOGRAD_NUMERICS_REPORT (JSON) when it is set (measured on
the MI355X: out 1.00 of its fp16 rounding, dy_dx 0.65, first-order dx 0.42, table 0.32 f32 / 0.66 f16, second-order ddy
0.50, dx 0.38, table 0.57 f32 / 0.69 f16)."""
import json
import os

import numpy as np
import pytest
import torch

import grid_autograd_restatement as G
import neus_bwd_restatement as R
from oracle import neus_oracle as NO

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
GUARD = 64
GS_F16, GS_F32 = 0, 1
MODES = (("f32", 1.0), ("f32", 128.0), ("f16", 128.0))
N_LIST = (1, 63, 64, 65, 255, 256, 257, 4099)
SCENES = ("uniform", "clump", "ray", "faces", "corners")
FIRST = (("table",), ("dx",), ("table", "dx"))
SECOND = (("table",), ("dx",), ("ddy",), ("table", "dx", "ddy"))

_stats = {"ratio": {}}


@pytest.fixture(scope="module", autouse=True)
def _report(built_lib):
    yield
    out = os.environ.get("GRID_AUTOGRAD_NUMERICS_REPORT")
    if out:
        with open(out, "w") as f:
            json.dump(_stats, f, indent=1, sort_keys=True)


def _note(key, err, bnd):
    err, bnd = np.asarray(err, np.float64), np.asarray(bnd, np.float64)
    pos = bnd > 0
    r = float((err[pos] / bnd[pos]).max()) if pos.any() else 0.0
    _stats["ratio"][key] = max(_stats["ratio"].get(key, 0.0), r)


def _lib():
    from go_slam_amd import _lib as lib_mod
    return lib_mod


def _t(x):
    return torch.as_tensor(np.ascontiguousarray(x)).to(DEV).contiguous()


def _sentinel(n, dtype=torch.float32):
    return torch.full((n + GUARD,), NAN, dtype=dtype, device=DEV)


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


@pytest.fixture(scope="module")
def meta():
    return NO.grid_meta()


@pytest.fixture(scope="module")
def grids(meta):
    out = {}
    for kind, seed in (("flat", 0), ("init", 1)):
        g = G.table(kind, seed, meta)
        out[kind] = (g, _t(g))
    return out


def _within(got, want, tag, key):
    err = np.abs(got - want.v)
    bad = ~(err <= want.e)
    if bad.any():
        i = np.argwhere(bad)[0]
        raise AssertionError(f"{tag}: {key}: {int(bad.sum())} of {err.size} beyond the bound, first {i.tolist()}: got "
                             f"{got[tuple(i)]} want {want.v[tuple(i)]} bound {want.e[tuple(i)]}")
    _note(key, err, want.e)


# ---------------------------------------------------------------------------------------------------- gs_grid_encode ----
def _encode(x, grid, n, dydx=True):
    lib = _lib()
    out = _sentinel(n * 32, torch.float16)
    dd = _sentinel(n * 96)
    lib.check(lib.lib().gs_grid_encode(lib.ptr(x), lib.ptr(grid), lib.ptr(out), lib.ptr(dd if dydx else None), n,
                                       lib.stream_ptr(DEV)), "grid_encode")
    torch.cuda.synchronize()
    return out, dd


def _check_encode(xh, gh, gd, meta, tag):
    n = len(xh)
    x = _t(xh)
    want = G.encode(xh, gh, meta)
    out, dd = _encode(x, gd, n)
    assert bool(out[n * 32:].isnan().all()) and bool(dd[n * 96:].isnan().all()), f"{tag}: written past n rows"
    o = out[:n * 32].view(n, 32).double().cpu().numpy()
    d = dd[:n * 96].view(n, 32, 3).double().cpu().numpy()
    assert np.isfinite(o).all() and np.isfinite(d).all(), f"{tag}: not written everywhere"
    w32 = want["out32"]
    lo, hi = R.h16(w32.v - w32.e), R.h16(w32.v + w32.e)
    bad = ~((o >= lo) & (o <= hi))
    assert not bad.any(), (f"{tag}: out: {int(bad.sum())} outside one fp16 rounding of the fp32 interval, first "
                           f"{np.argwhere(bad)[0].tolist()}: {o[bad][0]} vs [{lo[bad][0]}, {hi[bad][0]}]")
    _note("encode.out", np.abs(o - want["out"].v), want["out"].e)
    _within(d, want["dy_dx"], tag, "encode.dy_dx")
    out2, dd2 = _encode(x, gd, n)
    assert torch.equal(_bits(out), _bits(out2)) and torch.equal(_bits(dd), _bits(dd2)), f"{tag}: two runs differ"
    out3, dd3 = _encode(x, gd, n, dydx=False)
    assert torch.equal(_bits(out), _bits(out3)) and bool(dd3.isnan().all()), f"{tag}: dy_dx = NULL changes the run"
    return dd[:n * 96].view(n, 32, 3)


# -------------------------------------------------------------------------------------------------- gs_grid_backward ----
def _backward(x, grid, dy, dy_scale, v, mode, want, n, meta):
    """one launch; the outputs not in `want` are passed as NULL (their buffers stay allocated, to show they stay clean)"""
    lib = _lib()
    total = int(meta["total"]) * 2
    tab = torch.zeros(total + GUARD, dtype=torch.float32 if mode[0] == "f32" else torch.float16, device=DEV)
    tab[total:] = NAN
    dx, ddy = _sentinel(n * 3), _sentinel(n * 32)
    p = lambda name, buf: lib.ptr(buf if name in want else None)
    rc = lib.lib().gs_grid_backward(lib.ptr(x), lib.ptr(grid), lib.ptr(dy), GS_F16 if dy.dtype == torch.float16 else GS_F32,
                                    dy_scale, lib.ptr(v), p("table", tab), GS_F32 if mode[0] == "f32" else GS_F16, mode[1],
                                    p("dx", dx), p("ddy", ddy), n, lib.stream_ptr(DEV))
    lib.check(rc, "grid_backward")
    torch.cuda.synchronize()
    return {"table": tab, "dx": dx, "ddy": ddy}


def _check_table(tab, want, meta, tag, key, idx_dev):
    total = int(meta["total"]) * 2
    assert bool(tab[total:].isnan().all()), f"{tag}: the table's guard was written"
    assert not want["overflow"].any(), f"{tag}: {int(want['overflow'].sum())} entries of the fp16 table may overflow"
    got = tab[idx_dev].double().cpu().numpy()
    assert np.isfinite(got).all(), f"{tag}: non-finite table entries"
    stray = int(torch.count_nonzero(tab[:total])) - int(np.count_nonzero(got))
    assert stray == 0, f"{tag}: {stray} entries that no record reaches are not 0"
    err = np.abs(got - want["value"])
    bad = ~(err <= want["bound"])
    if bad.any():
        i = int(np.nonzero(bad)[0][0])
        e = int(want["idx"][i])
        lvl = int(np.searchsorted(meta["offset"].astype(np.int64) * 2, e, "right") - 1)
        raise AssertionError(f"{tag}: table: {int(bad.sum())} entries beyond, first {e} (level {lvl}, k = "
                             f"{int(want['k'][i])}): got {got[i]} want {want['value'][i]} bound {want['bound'][i]}")
    _note(key, err, want["bound"])


def _check_backward(xh, gh, gd, dyh, dy_scale, vh, meta, tag, modes=MODES, combos=None, twice=True):
    """first order (vh None) or second order: every mode x every combination of requested outputs"""
    n = len(xh)
    x, dy = _t(xh), _t(dyh)
    v = None if vh is None else _t(vh)
    order = "first" if vh is None else "second"
    want = G.backward(xh, gh, dyh, dy_scale, v=vh, tables=list(modes), meta=meta)
    for mode in modes:
        wt = want["tables"][mode]
        idx_dev = _t(wt["idx"])
        for combo in (combos or (FIRST if vh is None else SECOND)):
            t = f"{tag} {order} {mode[0]} x{mode[1]:g} {'+'.join(combo)}"
            got = _backward(x, gd, dy, dy_scale, v, mode, combo, n, meta)
            if "table" in combo:
                _check_table(got["table"], wt, meta, t, f"{order}.table.{mode[0]}", idx_dev)
            else:
                assert int(torch.count_nonzero(got["table"][:-GUARD])) == 0, f"{t}: the table was written"
            for k, w in (("dx", 3), ("ddy", 32)):
                buf = got[k]
                if k in combo:
                    assert bool(buf[n * w:].isnan().all()), f"{t}: {k} written past n rows"
                    g = buf[:n * w].view(n, w).double().cpu().numpy()
                    assert np.isfinite(g).all(), f"{t}: {k} not written everywhere"
                    _within(g, want[k], t, f"{order}.{k}")
                else:
                    assert bool(buf.isnan().all()), f"{t}: {k} was passed as NULL and written"
            if twice and len(combo) > 1:
                again = _backward(x, gd, dy, dy_scale, v, mode, combo, n, meta)
                for k in ("dx", "ddy"):
                    assert torch.equal(_bits(got[k]), _bits(again[k])), f"{t}: two runs give different {k}"
    return want


def _ups(i):
    return G.UPSTREAMS[i % len(G.UPSTREAMS)]


def _case(name, n, kind, up, seed, meta, grids, **kw):
    dt, sc, lv, vk = up
    gh, gd = grids[kind]
    xh = G.scene(name, n, seed=seed, meta=meta)
    dyh, vh = G.upstream(len(xh), seed + 1, dt, sc, level=lv, v=vk)
    tag = f"{name} n={len(xh)} {kind} dy {dt} x{sc:g} v {vk}"
    _check_backward(xh, gh, gd, dyh, sc, None, meta, tag, **kw)
    _check_backward(xh, gh, gd, dyh, sc, vh, meta, tag, **kw)


@pytest.mark.parametrize("n", N_LIST)
@pytest.mark.parametrize("name", SCENES)
def test_encode(name, n, meta, grids):
    gh, gd = grids["flat"]
    _check_encode(G.scene(name, n, seed=n, meta=meta), gh, gd, meta, f"{name} n={n}")


@pytest.mark.parametrize("kind", ["flat", "init"])
def test_encode_one_point_and_initial_table(kind, meta, grids):
    gh, gd = grids[kind]
    _check_encode(G.scene("one", 1, seed=3, meta=meta), gh, gd, meta, f"one {kind}")
    for name in ("uniform", "ray", "corners"):
        _check_encode(G.scene(name, 4099, seed=4, meta=meta), gh, gd, meta, f"{name} n=4099 {kind}")


@pytest.mark.parametrize("n", N_LIST)
@pytest.mark.parametrize("name", SCENES)
def test_backward(name, n, meta, grids):
    """every table mode and output combination; the upstream variant rotates with the case, and n = 4099 runs all of
    them"""
    i = SCENES.index(name) + N_LIST.index(n)
    for j in (range(len(G.UPSTREAMS)) if n == 4099 else (i,)):
        _case(name, n, "flat", _ups(j), 100 + n, meta, grids)


def test_backward_one_point(meta, grids):
    for j in range(len(G.UPSTREAMS)):
        _case("one", 1, "flat", _ups(j), 7 + j, meta, grids)


@pytest.mark.parametrize("n", [257, 4099])
@pytest.mark.parametrize("name", ["uniform", "ray"])
def test_backward_initial_table(name, n, meta, grids):
    """tcnn's initial table U(-1e-4, 1e-4): corner differences of fp16 values with few significant bits"""
    _case(name, n, "init", _ups(n), 300 + n, meta, grids)


def test_backward_production_batch(meta, grids):
    """4096 rays x 72 samples of the ray scene, the upstream as the drop-in's fp16 path sends it (fp16 dy under a scale);
    the combination the drop-in sends under the reference's use: first order dx alone and table alone, second order all
    three"""
    gh, gd = grids["flat"]
    n = 4096 * G.RAY_SAMPLES
    xh = G.scene("ray", n, seed=12, meta=meta)
    dyh, vh = G.upstream(n, 13, "f16", 1.0 / 128)
    modes = (("f16", 128.0), ("f32", 1.0))
    _check_backward(xh, gh, gd, dyh, 1.0 / 128, None, meta, "production", modes=modes, combos=(("dx",), ("table",)))
    _check_backward(xh, gh, gd, dyh, 1.0 / 128, vh, meta, "production", modes=modes, combos=(("table", "dx", "ddy"),))
    _check_encode(xh, gh, gd, meta, "production")


@pytest.mark.parametrize("name", ["clump", "ray", "corners"])
def test_one_hot_levels(name, meta, grids):
    """only level l's two features of dy non-zero, for every l, at n = 4099: dx, ddy and the level's table slice within
    bounds, every other level's slice exactly 0 -- no fine level can cover a coarse one"""
    gh, gd = grids["flat"]
    n = 4099
    total = int(meta["total"]) * 2
    xh = G.scene(name, n, seed=21, meta=meta)
    modes = (("f32", 1.0), ("f16", 128.0))
    for l in range(NO.N_LEVELS):
        dyh, vh = G.upstream(n, 22, "f16" if l % 2 else "f32", level=l)
        a, b = G.level_slice(meta, l)
        for v in (None, vh):
            tag = f"{name} one-hot level {l}"
            want = _check_backward(xh, gh, gd, dyh, 1.0, v, meta, tag, modes=modes,
                                   combos=(("table", "dx") if v is None else ("table", "dx", "ddy"),), twice=False)
            for mode in modes:
                idx = want["tables"][mode]["idx"]
                assert idx.size and idx.min() >= a and idx.max() < b, f"{tag}: the restatement leaves the level's slice"
                tab = _backward(_t(xh), gd, _t(dyh), 1.0, None if v is None else _t(v), mode, ("table",), n, meta)["table"]
                assert int(torch.count_nonzero(tab[:a])) == 0 and int(torch.count_nonzero(tab[b:total])) == 0, \
                    f"{tag} {mode}: another level's slice is not exactly 0"
                assert int(torch.count_nonzero(tab[a:b])) > 0


@pytest.mark.parametrize("n", [1, 65, 4099])
@pytest.mark.parametrize("name", SCENES)
def test_backward_dv_is_the_forwards_dy_dx(name, n, meta, grids):
    """ddy with v a unit vector is dv[axis] itself (1 dv + 0 dv' + 0 dv''): bit-equal to gs_grid_encode's dy_dx, as the
    kernel's comment promises"""
    for kind in ("flat", "init"):
        gh, gd = grids[kind]
        xh = G.scene(name, n, seed=31 + n, meta=meta)
        x = _t(xh)
        _, dd = _encode(x, gd, n)
        dd = dd[:n * 96].view(n, 32, 3)
        dy = _t(G.upstream(n, 32)[0])
        for axis in range(3):
            v = torch.zeros(n, 3, device=DEV)
            v[:, axis] = 1.0
            ddy = _backward(x, gd, dy, 1.0, v, ("f32", 1.0), ("ddy",), n, meta)["ddy"][:n * 32].view(n, 32)
            assert torch.equal(_bits(ddy), _bits(dd[:, :, axis].contiguous())), f"{name} n={n} {kind} axis {axis}"


def test_backward_refusals(meta, grids):
    lib = _lib()
    L = lib.lib()
    gh, gd = grids["flat"]
    n = 65
    total = int(meta["total"]) * 2
    x = _t(G.scene("uniform", n, seed=41, meta=meta))
    dyh, vh = G.upstream(n, 42)
    dy, v = _t(dyh), _t(vh)
    tab = torch.zeros(total + GUARD, device=DEV)
    dx, ddy = _sentinel(n * 3), _sentinel(n * 32)
    st = lib.stream_ptr(DEV)
    P = lib.ptr
    call = lambda **k: L.gs_grid_backward(
        P(x), P(k.get("grid", gd)), P(dy), k.get("dyt", GS_F32), 1.0, P(k.get("v", v)), P(k.get("tab", tab)),
        k.get("tt", GS_F32), 1.0, P(k.get("dx", dx)), P(k.get("ddy", ddy)), k.get("n", n), st)
    assert call(v=None) != 0, "ddy without v accepted"
    assert call(grid=None, ddy=None) != 0, "dx without grid accepted"
    assert call(grid=None, dx=None) != 0, "ddy without grid accepted"
    for bad in (2, 7, -1):
        assert call(dyt=bad) != 0, f"dy dtype {bad} accepted"
        assert call(tt=bad) != 0, f"table dtype {bad} accepted"
    assert call(n=-1) != 0, "n < 0 accepted"
    assert call(n=0) == 0, "n == 0 refused"
    torch.cuda.synchronize()
    assert int(torch.count_nonzero(tab)) == 0 and bool(dx.isnan().all()) and bool(ddy.isnan().all()), \
        "a refused / empty call wrote"
    out, dd = _sentinel(n * 32, torch.float16), _sentinel(n * 96)
    assert L.gs_grid_encode(P(x), P(gd), P(out), P(dd), -1, st) != 0, "encode: n < 0 accepted"
    assert L.gs_grid_encode(P(x), P(gd), P(out), P(dd), 0, st) == 0, "encode: n == 0 refused"
    assert L.gs_grid_encode(P(x), None, P(out), P(dd), n, st) != 0, "encode: no grid accepted"
    torch.cuda.synchronize()
    assert bool(out.isnan().all()) and bool(dd.isnan().all()), "a refused / empty encode wrote"
