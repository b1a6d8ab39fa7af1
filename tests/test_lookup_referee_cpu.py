"""tests/lookup_referee.py judged on the CPU: the rounding chain stays inside the derived bound (so a correct kernel can
meet it), agrees bit for bit with the oracle's independently written restatement, with torch's own bilinear sampler, and
each wrong lookup a kernel could plausibly compute misses the assertions tests/test_lookup_numerics_gpu.py makes (the
bound |y - ref| <= hard_bound, the bit equality y == lookup_chain)."""
import numpy as np
import pytest
import torch

import lookup_referee as R


def _refs(c, radius=3):
    key = ("refs", radius)
    if key not in c:
        c[key] = R.lookup_ref(c["levels"], c["coords"], radius)
    return c[key]


@pytest.mark.parametrize("name", R.CASES)
def test_chain_stays_inside_the_hard_bound(name):
    """every element of every case, dtype and radius: the condition for a correct kernel to be able to meet the bound"""
    c = R.case(name)
    for radius in (3, 1):
        ref, mag, ssum = R.lookup_ref(c["levels"], c["coords"], radius) if radius != 3 else _refs(c)
        for dt in ("f16", "f32", "f64"):
            y = R.lookup_chain(c["levels"], c["coords"], radius, dt)
            q = R.ratio(y, ref, mag, ssum, dt)
            fin = np.isfinite(ref) & np.isfinite(mag)
            overflow = fin & ~np.isfinite(y.astype(np.float64))
            if dt == "f16":                                  # a partial sum of 65504-sized terms may overflow in fp16
                assert (np.abs(mag[overflow]) >= 65504.0).all()
                q = np.where(overflow, 0.0, q)
            else:
                assert not overflow.any()
            print(f"{name} r={radius} {dt}: largest |chain - ref| / bound {np.nanmax(q):.3f}, {int(overflow.sum())} overflows, "
                  f"{int((~fin).sum())} non-finite references")
            assert np.nanmax(q) <= 1.0
            assert np.isnan(y[~fin].astype(np.float64)).all() or c["regime"] == "extreme"
    if c["regime"] == "cancelling":
        ref, mag, _ = _refs(c)
        assert np.median(np.abs(ref[0]) / np.maximum(mag[0], 1e-30)) < 1e-2
    if c["regime"] == "extreme":
        ref, _, _ = _refs(c)
        bad = ~np.isfinite(ref)
        assert bad[R.INF_PIXEL].any() and bad[R.NAN_PIXEL].any() and bad.mean() < 0.05


@pytest.mark.parametrize("name", R.CASES)
def test_chain_equals_the_oracle_bit_for_bit(name):
    """two independently written restatements: oracle.droid_oracle.corr_index_forward level by level, fp16 (and the fp32
    and fp64 element paths), radius 3 and 2"""
    from oracle import droid_oracle as O
    c = R.case(name)
    n, h1, w1 = c["n"], c["h1"], c["w1"]
    T = {"f16": torch.float16, "f32": torch.float32, "f64": torch.float64}
    for dt in ("f16", "f32", "f64"):
        for radius in (3, 2):
            rd = 2 * radius + 1
            for l, lv in enumerate(c["levels"]):
                coords_l = c["coords"] * np.float32(1.0 / (1 << l))
                vol = torch.from_numpy(lv).to(T[dt]).reshape(n, h1, w1, *lv.shape[2:])
                ct = torch.from_numpy(coords_l).reshape(n, h1, w1, 2).permute(0, 3, 1, 2).contiguous()
                want, = O.corr_index_forward(vol, ct, radius)
                want = want.reshape(n, rd * rd, h1 * w1).permute(0, 2, 1).numpy()
                got = R.lookup_chain([lv], coords_l, radius, dt)
                bad = ~R.same_bits(got, want)
                assert not bad.any(), f"{name} {dt} r={radius} level {l}: {int(bad.sum())} mismatches"


@pytest.mark.parametrize("name", R.CASES)
def test_ref_equals_grid_sample(name):
    """F.grid_sample(bilinear, zeros, align_corners=True) in float64 on the pixels with moderate coordinates: 2^-22 mag
    covers the fp32 weights against float64 ones.  The grid normalisation moves a position by up to 2^-50 of the plane's
    width, which mag does not cover where a weight is exactly 0 (integer coordinates: the sampler then takes 1e-15 of a
    neighbouring cell): 2^-40 of the level's largest finite cell is added for it."""
    c = R.case(name)
    ref, mag, _ = _refs(c)
    gs = R.grid_sample_ref(c["levels"], c["coords"], 3)
    sel = R.moderate(c)[..., None] & np.isfinite(ref) & np.isfinite(gs)
    assert (np.isfinite(ref) == np.isfinite(gs))[R.moderate(c)].all() or c["regime"] == "extreme"
    with np.errstate(invalid="ignore"):
        err = np.where(sel, np.abs(gs - ref), 0.0)
    cell = np.concatenate([np.full(49, np.abs(lv[np.isfinite(lv)]).max(), dtype=np.float64) for lv in c["levels"]])
    tol = 2.0 ** -22 * mag + 2.0 ** -40 * cell
    print(f"{name}: largest |grid_sample - ref| / tolerance {np.nanmax(np.where(sel, err / tol, 0.0)):.3f} over {int(sel.sum())}")
    assert sel.mean() > 0.5 and (np.where(sel, err, 0.0) <= np.where(sel, tol, 0.0)).all()


EXPECTED_MISS = {f: {"bound", "bits"} for f in R.FAULTS}
EXPECTED_MISS["fp32_accum"] = {"bits"}      # fewer roundings than the chain: inside the bound, caught by bit equality only


def missed(y, chain, ref, mag, ssum, dt):
    out = set()
    if not R.same_bits(y, chain).all():
        out.add("bits")
    if np.nanmax(R.ratio(y, ref, mag, ssum, dt)) > 1.0:
        out.add("bound")
    return out


@pytest.mark.parametrize("fault", R.FAULTS)
def test_wrong_lookups_miss_the_assertions(fault):
    """on the plain cases of a tile8 and a row-major map, fp16: which of the GPU test's two assertions each fault misses"""
    for name in ("16x32-plain", "15x20-plain"):
        c = R.case(name)
        ref, mag, ssum = _refs(c)
        chain = R.lookup_chain(c["levels"], c["coords"], 3, "f16")
        y = R.lookup_chain(c["levels"], c["coords"], 3, "f16", fault=fault)
        got = missed(y, chain, ref, mag, ssum, "f16")
        n_bits = int((~R.same_bits(y, chain)).sum())
        print(f"{fault} on {name}: misses {sorted(got)} ({n_bits} of {y.size} elements differ, largest ratio "
              f"{np.nanmax(R.ratio(y, ref, mag, ssum, 'f16')):.3g})")
        assert got == EXPECTED_MISS[fault]


def test_tile8_pack_round_trips():
    """through droid_backends.corr_untile8, including a 12-high level (a partial tile row) whose padding holds NaN"""
    from go_slam_amd.droid_backends import corr_untile8
    g = torch.Generator().manual_seed(5)
    for hl, wl in ((16, 32), (12, 24), (24, 48), (8, 16)):
        v = torch.randn(2, 3, 5, hl, wl, generator=g).half()
        packed = R.tile8_pack(v, pad=float("nan"))
        assert packed.shape == (2, 3, 5, ((hl + 7) // 8) * ((wl + 7) // 8) * 64)
        assert int(torch.isnan(packed).sum()) == 2 * 3 * 5 * (((hl + 7) // 8) * 8 - hl) * wl
        assert torch.equal(corr_untile8(packed, hl, wl), v)
        assert float(packed[0, 0, 0, 64 + 8 * 3 + 5]) == float(v[0, 0, 0, 3, 8 + 5])         # tile (0, 1), row 3, column 5


def test_backward_ref_is_the_adjoint_of_lookup_ref():
    c = R.case("15x20-plain")
    rng = np.random.default_rng(3)
    V = rng.standard_normal(c["levels"][0].shape)
    G = rng.standard_normal((c["n"], c["h1"] * c["w1"], 25))
    fwd, mag, _ = R.lookup_ref([V], c["coords"], 2)
    bwd, babs = R.backward_ref(c["coords"], G, 2, c["h2"], c["w2"])
    lhs, rhs = (fwd * G).sum(-1), (V * bwd).sum((-1, -2))
    scale = (mag * np.abs(G)).sum(-1)
    assert (np.abs(lhs - rhs) <= 64 * 2.0 ** -53 * scale + 1e-300).all()
    assert np.allclose((np.abs(V) * babs).sum((-1, -2)), (R.lookup_ref([np.abs(V)], c["coords"], 2)[0] * np.abs(G)).sum(-1),
                       rtol=1e-12)
