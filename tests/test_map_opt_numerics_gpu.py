"""The mapper step's Gram, reduction and AdamW kernels (go_slam_amd/csrc/map_opt.hip) against the fp64 restatement in
tests/map_opt_restatement.py, at the shapes, types and edges where they can go wrong.

Every kernel is called through the C ABI (ctypes), every output buffer is filled with a NaN sentinel first (plus a
guard region behind it), and the checks say what must be written and what must survive.  References are computed in
float64 from the kernels' own fp16 / fp32 inputs.  u = 2^-24.

  gs_map_gram        every workgroup's partial = the fp64 product over ITS row range (R.gram_split), per entry within
                     2 (D + 2) u sum |a_i b_i|, D = 16 ceil(per / 8) + 8; empty workgroups write exact zeros; exactly
                     the formed entries are written (R.gram_written); two runs are bit-equal.
  gs_map_step_post   every slot within (2 ceil(m / 8) + 10) u sum |terms| (m = nchunk or nb), the loss within
                     (2 ceil(n / 256) + 12) u sum |terms|; d variance exactly 0 outside the clamp; the spare slot after
                     the loss untouched; unread Gram entries hold NaN, so a wrong index shows.
  gs_map_step_prep   counts exactly (NaN maximum for a NaN depth), counts_in verbatim, inv_s within 2 ulp, d_gerr within
                     1 ulp, d_invs = sqnorm = 0, step + 1, sdf_wt and the fragment gather bit-equal.
  gs_map_grad_sqnorm relative error <= (8 ceil(n8 / stride) + 8 + n32 / stride + 300) u; inf -> +inf, NaN -> NaN.
  gs_map_adamw_seg   K = 5 steps vs clip_grad_norm_ + AdamW: |x - x64| within the accumulated R.clip_adamw bounds for
                     p, m, v; p16 bit-equal to the kernel's own p in fp16; non-finite patterns equal.

The worst error-to-bound ratio of each kernel is written to $MAP_OPT_NUMERICS_REPORT (JSON) when it is set."""
import json
import os

import numpy as np
import pytest
import torch

import map_opt_restatement as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
GUARD = 64
HYPER = dict(lr16=1e-2, lr32=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.01, max_norm=35.0)
INV_SCALE = 1.0 / 128.0

_stats = {"ratio": {}}


@pytest.fixture(scope="module", autouse=True)
def _report(built_lib):
    yield
    out = os.environ.get("MAP_OPT_NUMERICS_REPORT")
    if out:
        with open(out, "w") as f:
            json.dump(_stats, f, indent=1, sort_keys=True)


def _note(key, err, bnd):
    """record max(err / bnd) (err must be 0 wherever bnd is 0) and return it"""
    err = torch.as_tensor(err, dtype=torch.float64)
    bnd = torch.as_tensor(bnd, dtype=torch.float64, device=err.device)
    assert bool((err[bnd == 0] == 0).all()), f"{key}: nonzero error where the bound is 0"
    pos = bnd > 0
    r = float((err[pos] / bnd[pos]).max()) if bool(pos.any()) else 0.0
    _stats["ratio"][key] = max(_stats["ratio"].get(key, 0.0), r)
    return r


def _lib():
    from go_slam_amd import _lib as lib_mod
    return lib_mod


def _sentinel(n, dtype=torch.float32):
    return torch.full((n + GUARD,), NAN, dtype=dtype, device=DEV)


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


# ------------------------------------------------------------------------------------------------------ gs_map_gram ----
GRAM_ROWS = [16, 1008, 1024, 1040, 2048, 67600, 262144, 263232, 294912, 2359296]


def _gram_rows(n_rows, kind, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    if kind == "large":
        r = (torch.rand(n_rows, 160, generator=g, device=DEV) * 500.0 - 250.0).half()
    else:
        r = torch.randn(n_rows, 160, generator=g, device=DEV).half()
    if kind == "cancel":
        # pairs of rows equal but for the sign of columns 0..39: every product of a column < 40 with a column >= 40
        # cancels exactly in the pair's sum (Sigma ab = 0 for those entries, Sigma |ab| large)
        r = r.view(n_rows // 2, 2, 160)
        r[:, 1] = r[:, 0]
        r[:, 1, :40] = -r[:, 0, :40]
        r = r.view(n_rows, 160)
    else:                                               # the backward's layout: [.. x y z 1 0 0 0 0 ..]
        r[:, 35] = 1.0
        r[:, 36:40] = 0.0
    return r.contiguous()


def _run_gram(rows):
    lib = _lib()
    L = lib.lib()
    n_rows = rows.shape[0]
    nb = L.gs_map_gram_blocks(n_rows)
    out = torch.full((nb * 40 * 160 + GUARD,), NAN, dtype=torch.float32, device=DEV)
    lib.check(L.gs_map_gram(lib.ptr(rows), n_rows, lib.ptr(out), lib.stream_ptr(DEV)), "map_gram")
    torch.cuda.synchronize()
    assert bool(out[nb * 40 * 160:].isnan().all()), "gs_map_gram wrote past its partials"
    return out[:nb * 40 * 160].view(nb, 40, 160)


# (the largest shape with the real layout only)
GRAM_CASES = [(n, k) for n in GRAM_ROWS for k in ("real", "cancel", "large") if k == "real" or n <= 294912]


@pytest.mark.parametrize("n_rows,kind", GRAM_CASES)
def test_gram_partials_per_workgroup(n_rows, kind):
    L = _lib().lib()
    split = R.gram_split(n_rows)
    assert L.gs_map_gram_blocks(n_rows) == len(split)
    rows = _gram_rows(n_rows, kind, seed=n_rows % 9973 + len(kind))
    got = _run_gram(rows)
    W = R.gram_written().to(DEV)
    assert bool(got[:, ~W].isnan().all()), "an entry outside the formed blocks was written"
    assert bool(got[:, W].isfinite().all()), "a formed entry was not written"
    G64, A64 = R.gram_partials(rows)
    err = (got.double() - G64).abs()[:, W]
    bnd = R.gram_bound(n_rows, A64)[:, W]
    bad = err > bnd
    if bool(bad.any()):
        b, e = [int(x) for x in torch.nonzero(bad)[0]]
        raise AssertionError(f"{n_rows} rows ({kind}): {int(bad.sum())} entries beyond the bound, first workgroup {b} "
                             f"rows {split[b]}: got {float(got[:, W][b, e])} want {float(G64[:, W][b, e])} "
                             f"bound {float(bnd[b, e])}")
    _note("gram", err, bnd)
    for b, (lo, hi) in enumerate(split):
        if lo == hi:
            assert bool((got[b][W] == 0).all()), f"empty workgroup {b} did not write zeros"
    again = _run_gram(rows)
    assert torch.equal(_bits(again), _bits(got)), "two runs of gs_map_gram differ"


# ------------------------------------------------------------------------------------------------ gs_map_step_post ----
SF = 10.0
VAR = {"low": -2.0, "mid": 0.3, "high": 1.5}           # exp(var * 10): 2e-9 (clamped), 20, 3.3e6 (clamped)


def _run_post(gram, mlp_partial, d_invs, variance, inv_s, loss_rays, gerr, w_eik, s, counts):
    """g32 [ND + 1] from gs_map_step_post; gram / mlp_partial / loss_rays / gerr are device tensors (loss_rays and gerr
    may be longer than n: NaN guards the kernel must not read)"""
    lib = _lib()
    L = lib.lib()
    n = int(counts[3])
    sc = torch.tensor([d_invs, variance, inv_s], dtype=torch.float32, device=DEV)   # (alive until the kernel has run)
    cnt = torch.tensor(counts[:3], dtype=torch.float32, device=DEV)
    g32 = _sentinel(R.ND + 2)
    lib.check(L.gs_map_step_post(lib.ptr(gram), gram.shape[0], INV_SCALE, lib.ptr(mlp_partial), mlp_partial.shape[0],
                                 lib.ptr(sc[0:1]), lib.ptr(sc[1:2]), lib.ptr(sc[2:3]), SF, lib.ptr(loss_rays),
                                 lib.ptr(gerr), n, w_eik, s, lib.ptr(cnt), lib.ptr(g32), lib.stream_ptr(DEV)),
              "map_step_post")
    torch.cuda.synchronize()
    assert bool(g32[R.ND + 1:].isnan().all()), "the spare slot after the loss (or beyond) was written"
    return g32[:R.ND + 1].double().cpu().numpy()


def _post_inputs(nchunk, nb, n, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    W = R.gram_written().to(DEV)
    mag = 10.0 ** torch.randint(-2, 3, (40, 160), generator=g, device=DEV)
    gram = torch.randn(nchunk, 40, 160, generator=g, device=DEV) * mag * 128.0
    gram = torch.where(W, gram, torch.full_like(gram, NAN)).contiguous()      # unformed entries: must not be read
    mlp = (torch.randn(nb, R.N_MLP, generator=g, device=DEV) * 64.0).contiguous()
    loss_rays = _sentinel(n)
    gerr = _sentinel(n)
    loss_rays[:n] = torch.rand(n, generator=g, device=DEV) * 2.0 - 0.5
    gerr[:n] = torch.rand(n, generator=g, device=DEV) * 3.0
    return gram, mlp, loss_rays, gerr


def _check_post(got, want, bnd, what):
    assert R.same_nonfinite(got, want), f"{what}: non-finite pattern differs"
    ok = np.isfinite(want)
    err = np.abs(got[ok] - want[ok])
    bad = err > bnd[ok]
    if bad.any():
        i = np.flatnonzero(ok)[np.flatnonzero(bad)[:6]]
        raise AssertionError(f"{what}: {int(bad.sum())} slots beyond the bound at {i}: got {got[i]} want {want[i]} "
                             f"bound {bnd[i]}")
    return err, bnd[ok]


def _post_cases():
    nchunks = [1, 7, 8, 9, 63, 64, 65, 255, 256]
    nbs = [1, 7, 9, 64, 65, 330, "mlp32k"]
    ns = [0, 1, 255, 2047, 2049, 32768]
    regimes = ["low", "mid", "high"]
    return [(nchunks[i], nbs[i % len(nbs)], ns[i % len(ns)], regimes[i % len(regimes)]) for i in range(len(nchunks))]


@pytest.mark.parametrize("nchunk,nb,n,regime", _post_cases())
def test_step_post_against_fp64(nchunk, nb, n, regime):
    L = _lib().lib()
    if nb == "mlp32k":
        nb = L.gs_mlp_backward_blocks(32768 * 72)
        assert nb > 0
    gram, mlp, loss_rays, gerr = _post_inputs(nchunk, nb, n, seed=nchunk * 1000 + n)
    d_invs, var, w_eik, s = R.f32(-0.37), VAR[regime], R.f32(0.1), 72
    inv_s = R.f32(R.inv_s(var, SF))
    counts = [float(n // 2), float(n), 5.0, n]
    got = _run_post(gram, mlp, d_invs, var, inv_s, loss_rays, gerr, w_eik, s, counts)
    want, bnd = R.post(gram.double().cpu().numpy(), INV_SCALE, mlp.double().cpu().numpy(), d_invs, R.f32(var), inv_s,
                       SF, loss_rays[:n].double().cpu().numpy(), gerr[:n].double().cpu().numpy(), w_eik, s,
                       np.array(counts[:3]))
    what = f"post nchunk={nchunk} nb={nb} n={n} {regime}"
    assert np.isfinite(got[:R.OFF_LOSS]).all(), f"{what}: a gradient slot was not written"
    if regime != "mid":
        assert got[R.OFF_VAR] == 0.0, f"{what}: d variance outside the clamp must be exactly 0"
    else:
        assert got[R.OFF_VAR] != 0.0
    if n == 0:
        assert np.isnan(want[R.OFF_LOSS])       # the eikonal mean over no rays: 0 / 0, as torch's mean of nothing
    err, b = _check_post(got, want, bnd, what)
    ok = np.isfinite(want)
    sl = {"post_mlp": slice(0, R.N_MLP), "post_dense": slice(R.OFF_W, R.OFF_VAR),
          "post_var": slice(R.OFF_VAR, R.OFF_VAR + 1), "post_loss": slice(R.OFF_LOSS, R.OFF_LOSS + 1)}
    full_err = np.zeros(R.ND + 1)
    full_err[ok] = err
    for key, s_ in sl.items():
        if ok[s_].all():
            _note(key, full_err[s_], bnd[s_])


def test_gram_then_post_composed():
    """gs_map_gram -> gs_map_step_post on 294912 rows (4096 rays x 72 samples) vs post(gram(rows)) in fp64"""
    L = _lib().lib()
    n_rows, n = 294912, 4096
    rows = _gram_rows(n_rows, "real", seed=5)
    partial = _run_gram(rows)
    nb = L.gs_mlp_backward_blocks(n_rows)
    _, mlp, loss_rays, gerr = _post_inputs(1, nb, n, seed=6)
    d_invs, var, w_eik, s = R.f32(0.25), VAR["mid"], R.f32(0.1), 72
    inv_s = R.f32(R.inv_s(var, SF))
    counts = [4000.0, float(n), 5.0, n]
    got = _run_post(partial, mlp, d_invs, var, inv_s, loss_rays, gerr, w_eik, s, counts)
    G64, A64 = R.gram_partials(rows)
    args = (INV_SCALE, mlp.double().cpu().numpy(), d_invs, R.f32(var), inv_s, SF,
            loss_rays[:n].double().cpu().numpy(), gerr[:n].double().cpu().numpy(), w_eik, s, np.array(counts[:3]))
    want, _ = R.post(G64.cpu().numpy(), *args)
    _, bnd = R.post(A64.cpu().numpy(), *args)           # the summation bound with sum |a_i b_i| as the terms
    bnd[R.OFF_W:R.OFF_VAR] += R.post_dense(R.gram_bound(n_rows, A64).sum(0).cpu().numpy()) * INV_SCALE
    err, b = _check_post(got, want, bnd, "gram -> post")
    _note("gram_post_composed", err[R.OFF_W:R.OFF_VAR], b[R.OFF_W:R.OFF_VAR])


# ------------------------------------------------------------------------------------------------ gs_map_step_prep ----
def _prep_depths(n, nan_at, seed):
    rng = np.random.default_rng(seed)
    d = rng.uniform(0.1, 6.0, n).astype(np.float32)
    kind = rng.integers(0, 8, n)
    d[kind == 0] = 0.0
    d[kind == 1] = -rng.uniform(0.1, 3.0, int((kind == 1).sum()))
    if n > 2:
        d[rng.integers(0, n)] = np.inf
        d[n - 1] = 7.5
    if nan_at is not None:
        d[nan_at] = np.nan
    return d


def _run_prep(depth, var, w_eik, s, counts_in=None, step0=41, seed=0):
    lib = _lib()
    L = lib.lib()
    from go_slam_amd.neus.tcnn_compat import _mlp_fragment_index32
    n = depth.shape[0]
    rng = np.random.default_rng(seed)
    rd = _sentinel(n)
    rd[:n] = torch.from_numpy(depth).to(DEV)
    varb = torch.tensor([var], dtype=torch.float32, device=DEV)
    cin = None if counts_in is None else torch.tensor(counts_in, dtype=torch.float32, device=DEV)
    counts, inv_s, d_gerr = _sentinel(3), _sentinel(1), _sentinel(n)
    d_invs, sq = _sentinel(1), _sentinel(1)
    step = torch.full((1 + GUARD,), step0, dtype=torch.int32, device=DEV)
    sdf_w = torch.from_numpy(rng.standard_normal((32, 35)).astype(np.float32)).to(DEV)
    sdf_wt = _sentinel(1024)
    mlp16 = torch.from_numpy(rng.standard_normal(10240).astype(np.float16)).to(DEV)
    frag = _mlp_fragment_index32(torch.device(DEV))
    assert frag.numel() == 20480
    wpack = _sentinel(20480, torch.float16)
    lib.check(L.gs_map_step_prep(lib.ptr(rd), n, lib.ptr(varb), SF, w_eik, s, lib.ptr(cin), lib.ptr(counts),
                                 lib.ptr(inv_s), lib.ptr(d_gerr), lib.ptr(d_invs), lib.ptr(sq), lib.ptr(step),
                                 lib.ptr(sdf_w), lib.ptr(sdf_wt), lib.ptr(mlp16), lib.ptr(frag), lib.ptr(wpack),
                                 lib.stream_ptr(DEV)), "map_step_prep")
    torch.cuda.synchronize()
    for name, t, k in (("counts", counts, 3), ("inv_s", inv_s, 1), ("d_gerr", d_gerr, n), ("d_invs", d_invs, 1),
                       ("sqnorm", sq, 1), ("sdf_wt", sdf_wt, 1024), ("mlp_wpack", wpack, 20480)):
        assert bool(t[k:].isnan().all()), f"gs_map_step_prep wrote past {name}"
    assert bool((step[1:] == step0).all())
    return dict(counts=counts[:3].double().cpu().numpy(), inv_s=inv_s[:1].cpu().numpy(), d_gerr=d_gerr[:n].cpu().numpy(),
                d_invs=float(d_invs[0]), sqnorm=float(sq[0]), step=int(step[0]), sdf_w=sdf_w.cpu().numpy(),
                sdf_wt=sdf_wt[:1024].cpu(), mlp16=mlp16.cpu().numpy(), frag=frag.cpu().numpy(), wpack=wpack[:20480].cpu())


PREP_CASES = [(0, None, 0.3), (1, None, -2.0), (1023, None, 1.5), (8192, None, 0.3), (8193, None, 0.9),
              (32768, None, 0.3), (8193, 8192, 0.3), (32768, 517, 0.3), (1, 0, 0.3)]


@pytest.mark.parametrize("n,nan_at,var", PREP_CASES)
def test_step_prep_against_restatement(n, nan_at, var):
    from go_slam_amd.neus.tcnn_compat import _pack_mlp_fragments
    depth = _prep_depths(n, nan_at, seed=n + 3)
    w_eik, s = R.f32(0.1), 72
    got = _run_prep(depth, var, w_eik, s, seed=n)
    want = R.prep(depth, R.f32(var), SF, w_eik, s, sdf_w=got["sdf_w"], mlp16=got["mlp16"], frag_index=got["frag"])
    what = f"prep n={n} nan_at={nan_at}"
    np.testing.assert_array_equal(got["counts"], want["counts"], err_msg=what)     # NaN == NaN here
    assert R.ulps32(got["inv_s"], want["inv_s"])[0] <= 2, (what, got["inv_s"], want["inv_s"])
    _stats["ratio"]["prep_inv_s_ulps"] = max(_stats["ratio"].get("prep_inv_s_ulps", 0),
                                             int(R.ulps32(got["inv_s"], want["inv_s"])[0]))
    if n:
        u = R.ulps32(got["d_gerr"], want["d_gerr"])
        assert u.max() <= 1, (what, got["d_gerr"][:4], want["d_gerr"][:4])
    assert got["d_invs"] == 0.0 and got["sqnorm"] == 0.0 and got["step"] == 42, what
    assert torch.equal(_bits(got["sdf_wt"]), _bits(torch.from_numpy(want["sdf_wt"]))), what
    ref_pack = _pack_mlp_fragments(torch.from_numpy(got["mlp16"])).reshape(-1)
    assert torch.equal(_bits(got["wpack"]), _bits(ref_pack)), what
    assert np.array_equal(want["mlp_wpack"].view(np.int16), ref_pack.numpy().view(np.int16))


def test_step_prep_copies_counts_in_verbatim():
    depth = _prep_depths(1023, 5, seed=9)               # ignored: counts_in wins (a NaN depth included)
    cin = [np.float32(3.0), np.float32(4096.0), np.float32(np.nan)]
    got = _run_prep(depth, 0.3, R.f32(0.1), 72, counts_in=cin)
    assert np.array_equal(got["counts"][:2], [3.0, 4096.0]) and np.isnan(got["counts"][2])
    want = R.prep(depth, R.f32(0.3), SF, R.f32(0.1), 72, counts_in=cin)
    assert R.ulps32(got["d_gerr"], want["d_gerr"]).max() <= 1
    cin = [np.float32(7.0), np.float32(9.5), np.float32(-1.25)]
    got = _run_prep(depth, 0.3, R.f32(0.1), 72, counts_in=cin)
    assert got["counts"].tolist() == [7.0, 9.5, -1.25]


# ---------------------------------------------------------------------------------------------- gs_map_grad_sqnorm ----
def _slice(n16, G):
    return -(-n16 // (8 * G)) * 8


TABLE = 12599920
SQ_N16 = [0, 8, 13, 8 * 65536 * 8 - 8, 8 * 65536 * 8, 8 * 65536 * 8 + 29, TABLE] + [_slice(TABLE, G) for G in (2, 3, 8)]


def _grad16(n, seed, scale=4000.0):
    """loss-scaled fp16 gradients with subnormals and +-65504 sprinkled in"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = (torch.randn(n, generator=g, device=DEV) * scale).half()
    if n >= 8:
        x[n // 3] = 65504.0
        x[n // 2] = -65504.0
        x[1] = 2.0 ** -24
        x[n - 1] = -(2.0 ** -20)
        x[n // 5] = 6.0e-5                                # the largest fp16 subnormals
    return x


def _run_sqnorm(g16, g32, init=0.0):
    lib = _lib()
    L = lib.lib()
    out = _sentinel(1)
    out[0] = init
    lib.check(L.gs_map_grad_sqnorm(lib.ptr(g16), g16.numel(), INV_SCALE, lib.ptr(g32), g32.numel(), lib.ptr(out),
                                   lib.stream_ptr(DEV)), "map_grad_sqnorm")
    torch.cuda.synchronize()
    assert bool(out[1:].isnan().all())
    return float(out[0])


@pytest.mark.parametrize("n16", SQ_N16)
@pytest.mark.parametrize("n32", [0, 1, 11492])
def test_grad_sqnorm_against_fp64(n16, n32):
    g16 = _grad16(n16, seed=n16 % 100003 + n32)
    g32 = torch.randn(n32, generator=torch.Generator(device=DEV).manual_seed(n32), device=DEV) * 3.0
    init = 0.75
    got = _run_sqnorm(g16, g32, init)
    want = init + float((g16.double() * INV_SCALE).pow(2).sum() + g32.double().pow(2).sum())
    rel = R.sqnorm_rel_bound(n16, n32)
    err = abs(got - want)
    assert err <= rel * want, (n16, n32, got, want, err / want, rel)
    _note("sqnorm", err, rel * want)


@pytest.mark.parametrize("special,where", [(np.inf, "g16"), (-np.inf, "g16"), (np.nan, "g16"), (np.inf, "g32"),
                                           (np.nan, "g32")])
def test_grad_sqnorm_nonfinite(special, where):
    n16, n32 = 8 * 65536 * 8 + 29, 11492
    g16 = _grad16(n16, seed=3)
    g32 = torch.randn(n32, device=DEV)
    if where == "g16":
        g16[n16 - 2] = special                           # (in the n16 % 8 tail)
        g16[12345] = special
    else:
        g32[n32 - 1] = special
    got = _run_sqnorm(g16, g32)
    assert (np.isnan(got) if np.isnan(special) else got == np.inf), (special, where, got)


# ------------------------------------------------------------------------------------------------ gs_map_adamw_seg ----
def _h32():
    return {k: R.f32(v) for k, v in HYPER.items()}


def _adamw_grads(n16, n32, K, norm, seed, special=None):
    """K steps of (g16 loss-scaled fp16 [n16], g32 fp32 [n32]) with total unscaled norm ~ `norm`"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for k in range(K):
        a = torch.randn(n16, generator=g, dtype=torch.float64)
        b = torch.randn(n32, generator=g, dtype=torch.float64)
        nrm = float(torch.cat([a, b]).norm()) or 1.0
        a, b = a * (norm / nrm), b * (norm / nrm)
        g16 = (a / INV_SCALE).half()
        g32 = b.float()
        if special is not None and k == 1:
            if special == "inf":
                if n16:
                    g16[n16 // 2] = np.inf
                else:
                    g32[n32 // 2] = np.inf
            else:
                if n32:
                    g32[n32 - 1] = np.nan
                else:
                    g16[n16 - 1] = np.nan
        out.append((g16, g32))
    return out


def _adamw_run(n16, n32, K=5, norm=100.0, clip=True, p16=True, step_dev=False, step0=1, special=None, slice_of=None,
               seed=0):
    """K steps of gs_map_adamw_seg vs R.clip_adamw; returns the worst ratios.  slice_of = G: the table segment is
    rank 1's slice of a G-way sharded table of n16 entries (buffers of the whole table, the slice at its offset)."""
    lib = _lib()
    L = lib.lib()
    h = _h32()
    rng = np.random.default_rng(seed)
    if slice_of is not None:
        sl = _slice(n16, slice_of)
        total, lo = sl * slice_of, sl
        n16 = sl
    else:
        total, lo = n16, 0
    p0 = rng.standard_normal(total).astype(np.float32)
    pd0 = rng.standard_normal(n32).astype(np.float32)
    if step0 > 1:                                       # a long run's state
        m0 = (rng.standard_normal(n16) * 0.05).astype(np.float32)
        v0 = (rng.random(n16) * 1e-3).astype(np.float32)
        md0 = (rng.standard_normal(n32) * 0.05).astype(np.float32)
        vd0 = (rng.random(n32) * 1e-3).astype(np.float32)
    else:
        m0, v0, md0, vd0 = (np.zeros(k, np.float32) for k in (n16, n16, n32, n32))
    P = _sentinel(total)
    P[:total] = torch.from_numpy(p0).to(DEV)
    M, V, Pd, Md, Vd = _sentinel(n16), _sentinel(n16), _sentinel(n32), _sentinel(n32), _sentinel(n32)
    M[:n16], V[:n16] = torch.from_numpy(m0).to(DEV), torch.from_numpy(v0).to(DEV)
    Pd[:n32], Md[:n32], Vd[:n32] = (torch.from_numpy(x).to(DEV) for x in (pd0, md0, vd0))
    P16, P16d = _sentinel(total, torch.float16), _sentinel(n32, torch.float16)
    G16 = _sentinel(total, torch.float16)
    sq = torch.zeros(1, dtype=torch.float32, device=DEV)
    sdev = torch.zeros(1, dtype=torch.int32, device=DEV)
    grads = _adamw_grads(n16, n32, K, norm, seed + 1, special)
    p_tab = P[lo:lo + n16]
    for k, (g16, g32) in enumerate(grads):
        G16[lo:lo + n16] = g16.to(DEV)
        g32d = g32.to(DEV)
        sq.fill_(R.f32(R.sqnorm(g16.numpy(), INV_SCALE, g32.numpy())))
        t = step0 + k
        sdev.fill_(t)
        lib.check(L.gs_map_adamw_seg(lib.ptr(p_tab), lib.ptr(M), lib.ptr(V), lib.ptr(P16[lo:lo + n16]) if p16 else None,
                                     lib.ptr(G16[lo:lo + n16]), n16, INV_SCALE, lib.ptr(Pd), lib.ptr(Md), lib.ptr(Vd),
                                     lib.ptr(P16d) if p16 else None, lib.ptr(g32d), n32, h["lr16"], h["lr32"], h["b1"],
                                     h["b2"], h["eps"], h["wd"], 0 if step_dev else t,
                                     lib.ptr(sdev) if step_dev else None, lib.ptr(sq) if clip else None, h["max_norm"],
                                     lib.stream_ptr(DEV)), "map_adamw_seg")
    torch.cuda.synchronize()
    what = f"adamw n16={n16} n32={n32} clip={clip} p16={p16} step_dev={step_dev} step0={step0} {special} slice={slice_of}"
    # nothing outside the segments was touched
    for name, t, k in (("m", M, n16), ("v", V, n16), ("pd", Pd, n32), ("md", Md, n32), ("vd", Vd, n32),
                       ("p16d", P16d, n32 if p16 else 0)):
        assert bool(t[k:].isnan().all()), f"{what}: {name} written past its end"
    assert bool(P[total:].isnan().all()) and bool(P16[total:].isnan().all())
    if slice_of is not None:
        outside = torch.cat([P[:lo], P[lo + n16:total]]).cpu()
        assert torch.equal(outside, torch.cat([torch.from_numpy(p0[:lo]), torch.from_numpy(p0[lo + n16:])])), what
        assert bool(P16[:lo].isnan().all()) and bool(P16[lo + n16:total].isnan().all()), what
    if not p16:
        assert bool(P16.isnan().all()) and bool(P16d.isnan().all()), f"{what}: a NULL fp16 copy was written"
    p_ref, m_ref, v_ref, bounds = R.clip_adamw(
        [p0[lo:lo + n16].astype(np.float64), pd0.astype(np.float64)],
        [[(g16.double() * INV_SCALE).numpy(), g32.double().numpy()] for g16, g32 in grads],
        [h["lr16"], h["lr32"]], betas=(h["b1"], h["b2"]), eps=h["eps"], weight_decay=h["wd"], max_norm=h["max_norm"],
        m=[m0, md0], v=[v0, vd0], step0=step0, clip=clip)
    got = [(p_tab.cpu(), M[:n16].cpu(), V[:n16].cpu(), P16[lo:lo + n16].cpu()),
           (Pd[:n32].cpu(), Md[:n32].cpu(), Vd[:n32].cpu(), P16d[:n32].cpu())]
    for seg in range(2):
        gp, gm, gv, g16c = got[seg]
        if p16:
            assert torch.equal(_bits(g16c), _bits(gp.half())), f"{what}: fp16 copy != p.half()"
        for name, x, ref, b in (("p", gp, p_ref[seg], bounds[seg][0]), ("m", gm, m_ref[seg], bounds[seg][1]),
                                ("v", gv, v_ref[seg], bounds[seg][2])):
            x = x.double().numpy()
            assert R.same_nonfinite(x, ref), \
                f"{what}: segment {seg} {name}: non-finite pattern {np.isnan(x).sum()} NaN vs {np.isnan(ref).sum()}"
            ok = np.isfinite(ref)
            err = np.abs(x[ok] - ref[ok])
            bad = err > b[ok]
            if bad.any():
                i = np.flatnonzero(bad)[:4]
                raise AssertionError(f"{what}: segment {seg} {name}: {int(bad.sum())} beyond the bound: got {x[ok][i]} "
                                     f"want {ref[ok][i]} bound {b[ok][i]}")
            if ok.any():
                _note("adamw_" + name, err, b[ok])
    return p_ref


ADAMW_N16 = [0, 8, 13, 4096 * 8 + 5]


@pytest.mark.parametrize("n16", ADAMW_N16)
@pytest.mark.parametrize("n32", [0, 1, 11492])
def test_adamw_seg_sizes_clip_active(n16, n32):
    _adamw_run(n16, n32, norm=100.0, seed=n16 + n32)


@pytest.mark.parametrize("n32", [0, 11492])
def test_adamw_seg_sharded_slice_at_its_offset(n32):
    _adamw_run(100000, n32, slice_of=3, seed=5)


@pytest.mark.parametrize("case", ["inactive", "no_clip", "no_p16", "step_dev", "step_1e4", "step_1e4_dev"])
def test_adamw_seg_modes(case):
    n16, n32 = 4096 * 8 + 5, 11492
    kw = dict(inactive=dict(norm=10.0), no_clip=dict(norm=100.0, clip=False), no_p16=dict(p16=False),
              step_dev=dict(step_dev=True), step_1e4=dict(step0=10000), step_1e4_dev=dict(step0=10000, step_dev=True))
    _adamw_run(n16, n32, seed=11, **kw[case])


@pytest.mark.parametrize("special", ["inf", "nan"])
@pytest.mark.parametrize("n16,n32", [(4096 * 8 + 5, 11492), (13, 0), (0, 1)])
def test_adamw_seg_nonfinite_gradient(special, n16, n32):
    p = _adamw_run(n16, n32, special=special, seed=17)
    if special == "nan":
        assert all(np.isnan(x).all() for x in p)     # clip_grad_norm_: a NaN norm makes every parameter NaN
    else:
        assert sum(int(np.isnan(x).sum()) for x in p) == 1
