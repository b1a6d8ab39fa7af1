"""The NeuS training backward's ray and point kernels (go_slam_amd/csrc/neus_bwd.hip) against the fp64 restatement in
tests/neus_bwd_restatement.py, per element, at the shapes, regimes and lane layouts where they can go wrong.

Every kernel is called through the C ABI (ctypes).  Every output buffer is filled with a NaN sentinel first and has a
guard region behind it; the table gradient and d_inv_s are accumulated (zeroed) but keep a NaN guard.  Checked:
  gs_neus_backward_rays    n in {1, 3, 4, 5, 4099} x s in {1, 2, 63, 64, 65, 72, 127, 128}, eight regimes (soft, one
                           opaque sample, several, alpha = 1 - 2^-24, runs of >= 7 opaque samples with T through the
                           subnormals to 0, alpha = 0, mixed mask, |z| ~ 1e3), each upstream term alone and all together:
                           every d_alpha / d_rgb / d_grad within its bound, nothing written past n s, two runs bit-equal;
                           s = 129 refused, n = 0 a no-op.
  gs_neus_backward_points  fp32 table and fp16 (tiny-cuda-nn) table, gs_neus_backward_points_binned; enc_aux on and off;
  (+ _binned)              rows f32, f16 contiguous and f16 at stride 160 (the product's layout: pad columns 0, pts[:, 3] =
                           1, rows past n s untouched); dX f32 and f16 (scaled); sdf_wt NULL and set; inv_s by value and
                           by device pointer.  Every row entry, every table entry (entries no record touches exactly 0)
                           and d_inv_s within the restatement's bound; pts bit-equal to the fp32 restatement; rows bit-equal
                           across two runs.  Gate-exception points may match any admissible gate combination.
  poisoned input           one NaN d_alpha at a live point whose clip gate is open: non-finite exactly where autograd of
                           the reference graph is -- d sdf of that point, the 8 x 16 corner entries of the point (d enc =
                           W^T d_out is NaN for both features, and NaN times a corner weight is NaN even where the weight
                           is 0), d_inv_s, and dw0 of the point iff its cos < 0.  (At a MASKED point the kernel's `x *
                           live` makes that point's d_out row NaN where the reference's constant sdf = 100 stops the NaN;
                           harmless: the reference's d variance is NaN there too, and clip_grad_norm_ then turns every
                           gradient of the step NaN in both.)
The worst error / bound ratio per output and the gate-exception counts are written to $NEUS_BWD_NUMERICS_REPORT (JSON)
when it is set."""
import json
import os

import numpy as np
import pytest
import torch

import neus_bwd_restatement as R
from oracle import neus_oracle as NO

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
GUARD = 64
LS = 128.0

_stats = {"ratio": {}, "gate_exceptions": {}}


@pytest.fixture(scope="module", autouse=True)
def _report(built_lib):
    yield
    out = os.environ.get("NEUS_BWD_NUMERICS_REPORT")
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


# -------------------------------------------------------------------------------------------- gs_neus_backward_rays ----
REGIMES = ("soft", "one_opaque", "opaque_several", "near_one", "opaque_run", "zero", "mixed_mask", "far_z")
SAMPLES = (1, 2, 63, 64, 65, 72, 127, 128)


def _run_rays(sc, n, s):
    lib = _lib()
    L = lib.lib()
    ins = [_t(sc["alpha"]), _t(sc["rgb"]), _t(sc["z_mid"]), _t(sc["grad"]), _t(sc["mask"].astype(np.uint8))]
    ups = [_t(sc[k]) for k in R.UPSTREAM]
    outs = [_sentinel(n * s), _sentinel(n * s * 3), _sentinel(n * s * 3)]
    lib.check(L.gs_neus_backward_rays(*[lib.ptr(x) for x in ins + ups + outs], n, s, lib.stream_ptr(DEV)), "rays")
    torch.cuda.synchronize()
    return outs


def _check_rays(sc, n, s, tag):
    outs = _run_rays(sc, n, s)
    want = R.ray_bwd(**sc)
    sizes = {"d_alpha": n * s, "d_rgb": n * s * 3, "d_grad": n * s * 3}
    for (k, x), o in zip(want.items(), outs):
        m = sizes[k]
        assert bool(o[m:].isnan().all()), f"{tag}: {k} written past n s"
        got = o[:m].double().cpu().numpy()
        assert np.isfinite(got).all(), f"{tag}: {k} not written (or not finite)"
        err = np.abs(got - x.v.reshape(-1))
        bnd = x.e.reshape(-1)
        bad = err > bnd
        if bad.any():
            i = int(np.nonzero(bad)[0][0])
            raise AssertionError(f"{tag}: {k}: {int(bad.sum())} beyond the bound, first {i}: got {got[i]} want "
                                 f"{x.v.reshape(-1)[i]} bound {bnd[i]}")
        _note("rays." + k, err, bnd)
    again = _run_rays(sc, n, s)
    for a, b in zip(outs, again):
        assert torch.equal(_bits(a), _bits(b)), f"{tag}: two runs differ"


@pytest.mark.parametrize("s", SAMPLES)
@pytest.mark.parametrize("n", [1, 3, 4, 5])
def test_ray_backward_small(n, s):
    for regime in REGIMES:
        base = R.ray_scene(n, s, regime, seed=n * 131 + s)
        for which in R.UPSTREAM + ("all",):
            _check_rays(R.only(base, which), n, s, f"n={n} s={s} {regime} {which}")


@pytest.mark.parametrize("s", SAMPLES)
def test_ray_backward_4099_rays(s):
    regimes = REGIMES if s in (64, 65, 72, 128) else ("soft", "opaque_run")
    for regime in regimes:
        _check_rays(R.ray_scene(4099, s, regime, seed=s), 4099, s, f"n=4099 s={s} {regime}")


def test_ray_backward_refuses_bad_shapes():
    lib = _lib()
    L = lib.lib()
    sc = R.ray_scene(2, 128, "soft")
    ins = [_t(sc["alpha"]), _t(sc["rgb"]), _t(sc["z_mid"]), _t(sc["grad"]), _t(sc["mask"].astype(np.uint8))]
    ups = [_t(sc[k]) for k in R.UPSTREAM]
    outs = [_sentinel(2 * 129 * 3) for _ in range(3)]
    args = [lib.ptr(x) for x in ins + ups + outs]
    assert L.gs_neus_backward_rays(*args, 1, 129, lib.stream_ptr(DEV)) != 0, "s = 129 accepted"
    assert L.gs_neus_backward_rays(*args, 0, 72, lib.stream_ptr(DEV)) == 0, "n = 0 refused"
    torch.cuda.synchronize()
    assert all(bool(o.isnan().all()) for o in outs), "a refused / empty call wrote"


# ------------------------------------------------------------------------------------------- gs_neus_backward_points ----
# entry, table, aux, rows (dtype, stride), dX f16, sdf_wt, inv_s on the device
VARIANTS = {
    "atomic32":          ("points", "f32", False, ("f32", 0), False, False, False),
    "atomic16_aux":      ("points", "f16", True, ("f16", 0), True, False, True),
    "binned_product":    ("binned", "f16", True, ("f16", 160), True, True, True),
    "binned_plain":      ("binned", "f16", False, ("f32", 0), False, False, False),
    "atomic32_aux_wide": ("points", "f32", True, ("f16", 160), True, False, False),
    "atomic16":          ("points", "f16", False, ("f32", 0), False, False, True),
}
SCENES = ("one", "soft", "hard3", "hard5", "lanes", "line")
WIDTH32 = {"d_out": 32, "lin_in": 35, "dw0": 35, "d_arg": 33, "pts": 3}
WIDTH16 = {"d_out": 32, "lin_in": 40, "dw0": 40, "d_arg": 40, "pts": 8}
COL160 = {"d_out": 0, "pts": 32, "lin_in": 40, "dw0": 80, "d_arg": 120}

_cache = {}


@pytest.fixture(scope="module")
def meta():
    return NO.grid_meta()


@pytest.fixture(scope="module")
def prm(meta):
    return R.params(0, meta)


@pytest.fixture(scope="module")
def dev_params(prm):
    W = prm["sdf_w"]
    wt = np.ascontiguousarray(W[:, 3:].reshape(32, 16, 2).transpose(1, 2, 0))   # [l][f][o] = W[o][3 + 2 l + f]
    return dict(grid=_t(prm["grid"]), sdf_w=_t(W), sdf_wt=_t(wt), color_B=_t(prm["color_B"]))


def _want(name, meta, prm, aux, dx16, rs, mode):
    key = (name, aux, dx16, rs, mode)
    if key not in _cache:
        sc = _cache.setdefault(("scene", name), R.scene(name, seed=7, meta=meta))
        P = R.prepare_scene(sc, prm, dx16=dx16, dx_scale=LS, aux=aux, row_scale=rs, meta=meta)
        _cache[key] = (P, R.point_bwd(P, "f32" if mode == "f32" else ("binned" if mode == "binned" else "f16"), LS))
    return _cache[("scene", name)], _cache[key]


def _run_points(sc, dp, var, meta, d_alpha=None):
    entry, table, aux, (rdt, stride), dx16, use_wt, inv_dev = var
    lib = _lib()
    L = lib.lib()
    n, s = sc["z_vals"].shape
    N = n * s
    total = int(meta["total"]) * 2
    tdt = torch.float32 if table == "f32" else torch.float16
    tab = torch.zeros(total + GUARD, dtype=tdt, device=DEV)
    tab[total:] = NAN
    dinv = torch.zeros(1 + GUARD, device=DEV)
    dinv[1:] = NAN
    r16 = rdt == "f16"
    rows_dt = torch.float16 if r16 else torch.float32
    if stride:
        mat = torch.full(((N + 2) * stride + GUARD,), NAN, dtype=rows_dt, device=DEV)
        bufs = {k: mat[c:] for k, c in COL160.items()}
    else:
        W = WIDTH16 if r16 else WIDTH32
        bufs = {k: _sentinel(N * W[k], rows_dt) for k in WIDTH32}
        mat = None
    dX = _t((sc["dX"] * np.float32(LS)).astype(np.float16)) if dx16 else _t(sc["dX"])
    inv_s = float(sc["inv_s"])
    inv_t = _t(np.array([inv_s], np.float32)) if inv_dev else None
    ea = _t(sc["enc_aux"]) if aux else None
    bound = np.asarray(R.BOUND, np.float32)
    da = sc["d_alpha"] if d_alpha is None else d_alpha
    ins = [_t(sc["rays_o"]), _t(sc["rays_d"]), _t(sc["z_vals"]), _t(sc["dists"]), dp["grid"], dp["sdf_w"],
           dp["color_B"]]
    pre = [lib.ptr(x) for x in ins] + [NAN if inv_dev else inv_s, lib.ptr(inv_t), bound.ctypes.data]
    pin = [_t(sc["sdf"]), _t(sc["grad"]), _t(sc["mask"]), _t(da), _t(sc["d_sdf"]), _t(sc["d_grad"]),
           _t(sc["d_gerr_ray"])]                       # (held until the kernel has run: the pointers must not alias)
    mid = [lib.ptr(x) for x in pin[:6]] + [lib.ptr(dX), 0 if dx16 else 1, LS if dx16 else 1.0, lib.ptr(pin[6]),
                                           lib.ptr(tab)]
    rows = [bufs[k].data_ptr() for k in ("d_out", "lin_in", "dw0", "d_arg", "pts")]
    rs = LS if r16 else 1.0
    keep = [ins, pin, inv_t, ea, dX, bound]
    if entry == "points":
        rc = L.gs_neus_backward_points(*pre, *mid, 1 if table == "f32" else 0, LS, *rows, 0 if r16 else 1, rs, stride,
                                       lib.ptr(dinv), n, s, lib.ptr(ea), lib.stream_ptr(DEV))
    else:
        nb = L.gs_neus_bin_workspace_bytes(N)
        ws = torch.full((nb,), 0xA5, dtype=torch.uint8, device=DEV)            # no initial state
        keep.append(ws)
        rc = L.gs_neus_backward_points_binned(*pre, *mid, LS, *rows, 0 if r16 else 1, rs, stride, lib.ptr(dinv), n, s,
                                              lib.ptr(ws), nb, lib.ptr(dp["sdf_wt"] if use_wt else None),
                                              lib.ptr(ea), lib.stream_ptr(DEV))
    lib.check(rc, "neus_backward_points")
    torch.cuda.synchronize()
    del keep
    return tab, dinv, bufs, mat


def _rows_of(bufs, mat, var, N):
    """{name: float64 [N, width]} and the pad checks"""
    _, _, _, (rdt, stride), _, _, _ = var
    out = {}
    if stride:
        M = mat[:(N + 2) * stride].view(N + 2, stride)
        assert bool(M[N:].isnan().all()), "rows past n s were written"
        assert bool(mat[(N + 2) * stride:].isnan().all()), "guard written"
        for k, c in COL160.items():
            out[k] = M[:N, c:c + WIDTH16[k]].double().cpu().numpy()
    else:
        W = WIDTH16 if rdt == "f16" else WIDTH32
        for k in WIDTH32:
            b = bufs[k]
            assert bool(b[N * W[k]:].isnan().all()), f"{k} written past n s"
            out[k] = b[:N * W[k]].view(N, W[k]).double().cpu().numpy()
    for k, x in out.items():
        assert np.isfinite(x).all(), f"row {k} not written everywhere"
    if rdt == "f16":
        assert (out["lin_in"][:, 35:] == 0).all() and (out["dw0"][:, 35:] == 0).all(), "lin_in / dw0 pad not zero"
        assert (out["d_arg"][:, 33:] == 0).all(), "d_arg pad not zero"
        assert (out["pts"][:, 3] == 1).all() and (out["pts"][:, 4:] == 0).all(), "pts pad not (1, 0, 0, 0, 0)"
    return out


def _check_rows(got, want, P, var, tag):
    _, _, _, (rdt, _), _, _, _ = var
    pts = P["pts"]
    exp_pts = R.h16(pts) if rdt == "f16" else pts
    assert np.array_equal(got["pts"][:, :3], exp_pts), f"{tag}: pts differ from the fp32 restatement"
    alt = {}
    for p, r in want["alt"]:
        alt.setdefault(p, []).append(r)
    for k, x in want["rows"].items():
        wv = x.v
        wb = R.round16(x).e if rdt == "f16" else x.e
        g = got[k][:, :wv.shape[1]]
        err = np.abs(g - wv)
        bad = (err > wb).any(1)
        for p in np.nonzero(bad)[0]:
            ok = False
            for r in alt.get(int(p), []):
                y = r[k]
                yb = R.round16(y).e if rdt == "f16" else y.e
                ok |= bool((np.abs(g[p] - y.v) <= yb).all())
            if not ok:
                c = int(np.nonzero(err[p] > wb[p])[0][0])
                raise AssertionError(f"{tag}: {k}[{p}, {c}] got {g[p, c]} want {wv[p, c]} bound {wb[p, c]} "
                                     f"({int(bad.sum())} points beyond)")
        okp = ~bad
        _note(f"rows.{k}.{rdt}", err[okp], wb[okp])


def _check_table(tab, dinv, want, var, meta, tag):
    total = int(meta["total"]) * 2
    assert bool(tab[total:].isnan().all()), f"{tag}: the table's guard was written"
    assert bool(dinv[1:].isnan().all()), f"{tag}: d_inv_s's guard was written"
    got = tab[:total].double().cpu().numpy()
    S, B = want["table"]
    touched = want["touched"]
    assert np.all(got[~touched] == 0.0), f"{tag}: {int((got[~touched] != 0).sum())} untouched entries nonzero"
    err = np.abs(got - S)
    bad = err > B
    if bad.any():
        i = int(np.nonzero(bad)[0][0])
        lvl = int(np.searchsorted(meta["offset"].astype(np.int64) * 2, i, "right") - 1)
        raise AssertionError(f"{tag}: table: {int(bad.sum())} entries beyond, first {i} (level {lvl}): got {got[i]} "
                             f"want {S[i]} bound {B[i]}")
    _note(f"table.{var[1] if var[0] == 'points' else 'binned'}", err[touched], B[touched])
    dv, db = want["d_inv_s"]
    g = float(dinv[0])
    assert abs(g - dv) <= db, f"{tag}: d_inv_s got {g} want {dv} bound {db}"
    _note("d_inv_s", [abs(g - dv)], [db])


def _case(name, vname, meta, prm, dp):
    var = VARIANTS[vname]
    entry, table, aux, (rdt, _), dx16, _, _ = var
    mode = "binned" if entry == "binned" else table
    sc, (P, want) = _want(name, meta, prm, aux, dx16, LS if rdt == "f16" else 1.0, mode)
    tag = f"{name}/{vname}"
    N = P["npt"]
    tab, dinv, bufs, mat = _run_points(sc, dp, var, meta)
    got = _rows_of(bufs, mat, var, N)
    _check_rows(got, want, P, var, tag)
    _check_table(tab, dinv, want, var, meta, tag)
    for k, c in want["exceptions"].items():
        _stats["gate_exceptions"][f"{name}.{k}"] = c
    tab2, dinv2, bufs2, mat2 = _run_points(sc, dp, var, meta)
    got2 = _rows_of(bufs2, mat2, var, N)
    for k in got:
        assert np.array_equal(got[k], got2[k]), f"{tag}: two runs give different {k} rows"


@pytest.mark.parametrize("vname", list(VARIANTS))
@pytest.mark.parametrize("name", SCENES)
def test_point_backward(name, vname, meta, prm, dev_params):
    _case(name, vname, meta, prm, dev_params)


@pytest.mark.parametrize("vname", ["binned_product", "atomic32"])
def test_point_backward_production_batch(vname, meta, prm, dev_params):
    """4099 rays x 72 samples along sorted depths (ragged: 4099 x 72 is not a multiple of 256)"""
    _case("big", vname, meta, prm, dev_params)


@pytest.mark.parametrize("vname", ["atomic32", "binned_product"])
def test_point_backward_poisoned_d_alpha(vname, meta, prm, dev_params):
    var = VARIANTS[vname]
    sc, (P, want) = _want("soft", meta, prm, var[2], var[4], LS if var[3][0] == "f16" else 1.0,
                          "binned" if var[0] == "binned" else var[1])
    N = P["npt"]
    da = sc["d_alpha"].copy()
    k = int(np.nonzero(P["on"] & (da != 0))[0][17])
    da[k] = np.float32(NAN)
    tab, dinv, bufs, mat = _run_points(sc, dev_params, var, meta, d_alpha=da)
    total = int(meta["total"]) * 2
    bad = ~torch.isfinite(tab[:total]).cpu().numpy()
    want_bad = np.zeros(total, bool)
    for l in range(NO.N_LEVELS):
        gi, _ = R.cells(P["view"][k:k + 1], meta["scale"][l])
        e = R.grid_corners(meta, l, gi)[0] + int(meta["offset"][l])
        want_bad[2 * e] = want_bad[2 * e + 1] = True
    assert np.array_equal(bad, want_bad), (f"non-finite table entries: {int(bad.sum())} (want the point's "
                                           f"{int(want_bad.sum())} corner entries)")
    assert not bool(torch.isfinite(dinv[0])), "d_inv_s finite"
    rdt, stride = var[3]
    W = WIDTH16 if rdt == "f16" else WIDTH32
    if stride:
        M = mat[:N * stride].view(N, stride)
        rows = {kk: M[:, c:c + W[kk]] for kk, c in COL160.items()}
    else:
        rows = {kk: bufs[kk][:N * W[kk]].view(N, W[kk]) for kk in WIDTH32}
    cos_neg = float(P["dir"][k] @ P["grad"][k]) < 0
    for kk, x in rows.items():
        nf = ~torch.isfinite(x).cpu().numpy()
        want_nf = np.zeros_like(nf)
        if kk == "d_out":
            want_nf[k, 0] = True
        if kk == "dw0" and cos_neg:
            want_nf[k, :35] = True
        assert np.array_equal(nf, want_nf), f"{kk}: non-finite at {np.argwhere(nf)[:5].tolist()}"
