"""The window lookups of csrc/corr_lookup.hip against tests/lookup_referee.py, per element and on every load path.

Every entry point is called through ctypes on the seeded cases of lookup_referee.case (five target maps x three volume
regimes, three edges with 0.5 / 4 / 40 px of noise, source maps of 5 x 7 and 9 x 8 pixels -- another size than the target
map --, fixed pixels at integers, half-integers, windows that just touch or just leave each border, +-1e6, 1e9, -3e38 and
+-1e-40).  The output is prefilled with a NaN sentinel of its own payload (every element must be overwritten) between two
guard regions (which must keep it), and every call runs twice and must give the same bits.  Each path asserts

    bits    y == lookup_chain, value for value and NaN for NaN (lookup_referee.same_bits): the contract's rounding sequence
    bound   |y - ref| <= hard_bound wherever the float64 reference is finite

and with them that a tap is non-finite exactly where the referee's is.  Nothing computed on the GPU acts as referee.

Paths (x = runs on that target map):                                   16x32  24x48  12x16  15x20  8x12
  pyr f16 planar           corr_pyramid_kernel<half, false>, __int128    x      x      x      x      x     (narrow: l >= 1..3)
  pyr f16 nhwc             coop kernel, clamped load + funnel shift      x      x      x      x      x
  pyr f16 nhwc tile8       coop kernel, straddled tiles, partial rows    x      x
  pyr f16 nhwc slots       slot = [4, 0, 2] of 5, the rest NaN           x      x      x      x      x
  pyr f16 nhwc tile8 slots                                               x      x
  pyr f32 planar / nhwc    element path / emit_nhwc's carries            x      x      x      x      x
  idx f16 / f32 / f64 r=3  levels 0 and 2 as single-level volumes        x      x      x      x      x
  idx f32 / f64 r=1, 2, 4; idx f16 r=1   corr_index_generic_kernel       x      x      x      x      x
  backward f32 / f64 r=3, 2   against the float64 adjoint, per element, and the adjoint identity per pixel

MEASURED (MI355X; over all cases of a path: runs, elements, largest |y - ref| / hard_bound, bit mismatches, non-finite
taps -- each of them non-finite in the referee too; none of these figures is a tolerance):
  pyr f16 planar                15 runs    460992 elements  largest ratio 0.621  mismatches 0  non-finite taps 161
  pyr f16 nhwc                  15 runs    460992 elements  largest ratio 0.621  mismatches 0  non-finite taps 161
  pyr f16 nhwc slots            15 runs    460992 elements  largest ratio 0.621  mismatches 0  non-finite taps 161
  pyr f32 planar                15 runs    460992 elements  largest ratio 0.801  mismatches 0  non-finite taps 160
  pyr f32 nhwc                  15 runs    460992 elements  largest ratio 0.801  mismatches 0  non-finite taps 160
  pyr f16 nhwc tile8             9 runs    272244 elements  largest ratio 0.621  mismatches 0  non-finite taps 97
  pyr f16 nhwc tile8 slots       9 runs    272244 elements  largest ratio 0.621  mismatches 0  non-finite taps 97
  idx f16 r=3 (levels 0, 2)     30 runs    230496 elements  largest ratio 0.597  mismatches 0  non-finite taps 81
  idx f32 r=3 (levels 0, 2)     30 runs    230496 elements  largest ratio 0.801  mismatches 0  non-finite taps 80
  idx f64 r=3 (levels 0, 2)     30 runs    230496 elements  largest ratio 0.000  mismatches 0  non-finite taps 80
  idx f32 r=1 / 2 / 4           15 runs each                    largest ratio 0.640 / 0.672 / 0.801  mismatches 0
  idx f64 r=1 / 2 / 4           15 runs each                    largest ratio 0.000  mismatches 0
  idx f16 r=1                   15 runs     21168 elements  largest ratio 0.480  mismatches 0  non-finite taps 40
  (fp16 has one non-finite tap more than fp32: one partial sum of 65504-sized terms overflows, in the chain as well.
   The fp64 ratio is 0 because the float64 reference sums in the chain's order; fp64 is judged by the bit equality.)
  backward f32 / f64, r = 3 / 2  20 runs  largest |B - ref| / bound 0.360, adjoint identity 0.113 of its bound,
                                           51 .. 96 of 105 / 216 slices wholly outside and exactly zero
  non-finite coordinates         5 maps   40851 / 51435 taps per map NaN, every other element bit-equal to the clean run"""
import ctypes

import numpy as np
import pytest
import torch

import lookup_referee as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64
T_DT = {"f16": torch.float16, "f32": torch.float32, "f64": torch.float64}
I_DT = {"f16": torch.int16, "f32": torch.int32, "f64": torch.int64}
GS_DT = {"f16": 0, "f32": 1, "f64": 2}
SENTINEL = {"f16": 0x7E5A, "f32": 0x7FC5A5A5, "f64": 0x7FF85A5A5A5A5A5A}       # quiet NaNs no arithmetic produces
ROWMAJOR, TILE8 = 0, 1


@pytest.fixture(autouse=True)
def _stop_after_a_device_error():
    """a failed assertion lets the next test run; a device error ends the session (nothing more is launched after it)"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as exc:
        pytest.exit(f"device error, stopping: {exc}", returncode=3)


# ------------------------------------------------------------------------------------------------ running an entry

def _twice(numel, dt, launch, prefill_zero=False):
    """launch(ptr) twice into sentinel-filled buffers with guards -> the body as a numpy array of dtype dt (flat)"""
    runs = []
    for _ in range(2):
        buf = torch.full((numel + 2 * GUARD,), SENTINEL[dt], dtype=I_DT[dt], device=DEV)
        if prefill_zero:
            buf[GUARD:GUARD + numel] = 0
        launch(ctypes.c_void_p(buf.data_ptr() + GUARD * buf.element_size()))
        torch.cuda.synchronize()
        host = buf.cpu()
        assert bool((host[:GUARD] == SENTINEL[dt]).all()) and bool((host[GUARD + numel:] == SENTINEL[dt]).all()), \
            "the kernel wrote outside its output"
        body = host[GUARD:GUARD + numel]
        if not prefill_zero:
            assert bool((body != SENTINEL[dt]).all()), f"{int((body == SENTINEL[dt]).sum())} elements were never written"
        runs.append(body)
    assert torch.equal(runs[0], runs[1]), "two runs of the same call differ"
    return runs[0].view(T_DT[dt]).numpy()


def _dev_levels(c, dt, tile8):
    """the four levels on the device as [n,P,plane] (tile8: levels 0-1 packed on the host, partial tiles padded with NaN)"""
    out = []
    for l, lv in enumerate(c["levels"]):
        t = torch.from_numpy(lv).to(T_DT[dt])
        t = R.tile8_pack(t, pad=float("nan")) if tile8 and l < 2 else t.reshape(t.shape[0], t.shape[1], -1)
        out.append(t.contiguous())
    return out


def run_pyramid(c, coords, dt, nhwc, layout=ROWMAJOR, slots=False):
    """gs_corr_lookup_pyramid[_slots] -> [n,P,196]"""
    from go_slam_amd import _lib
    n, P = c["n"], c["h1"] * c["w1"]
    vols = _dev_levels(c, dt, layout == TILE8)
    slot = None
    if slots:
        pool = []
        for v in vols:
            s = torch.full((R.CAPACITY,) + tuple(v.shape[1:]), float("nan"), dtype=v.dtype)
            s[R.SLOTS] = v
            pool.append(s)
        vols = pool
        slot = torch.tensor(R.SLOTS, dtype=torch.int64, device=DEV)
    vols = [v.to(DEV) for v in vols]
    cd = torch.from_numpy(np.ascontiguousarray(coords)).to(DEV)
    L = _lib.lib()

    def launch(out):
        tail = (n, c["h1"], c["w1"], c["h2"], c["w2"], 3, GS_DT[dt], int(nhwc), layout, _lib.stream_ptr(DEV))
        if slots:
            rc = L.gs_corr_lookup_pyramid_slots(*[_lib.ptr(v) for v in vols], _lib.ptr(slot), _lib.ptr(cd), out, *tail)
        else:
            rc = L.gs_corr_lookup_pyramid(*[_lib.ptr(v) for v in vols], _lib.ptr(cd), out, *tail)
        _lib.check(rc, "corr_lookup_pyramid")

    y = _twice(n * P * 196, dt, launch)
    return y.reshape(n, P, 196) if nhwc else y.reshape(n, 196, P).transpose(0, 2, 1)


def run_index(c, coords_l, level, dt, radius):
    """gs_corr_index_forward on level `level` as a single-level volume -> [n,P,rd*rd]"""
    from go_slam_amd import _lib
    n, P, rd = c["n"], c["h1"] * c["w1"], 2 * radius + 1
    lv = c["levels"][level]
    vol = torch.from_numpy(lv).to(T_DT[dt]).contiguous().to(DEV)
    cd = torch.from_numpy(np.ascontiguousarray(coords_l.transpose(0, 2, 1))).to(DEV)                # [n,2,P]

    def launch(out):
        rc = _lib.lib().gs_corr_index_forward(_lib.ptr(vol), _lib.ptr(cd), out, n, c["h1"], c["w1"], lv.shape[2], lv.shape[3],
                                              radius, GS_DT[dt], _lib.stream_ptr(DEV))
        _lib.check(rc, "corr_index_forward")

    return _twice(n * rd * rd * P, dt, launch).reshape(n, rd * rd, P).transpose(0, 2, 1)


def run_backward(c, coords, grad, dt, radius):
    """gs_corr_index_backward: grad [n,P,rd*rd] (dtype values) -> vol_grad [n,P,h2,w2] from a zeroed buffer"""
    from go_slam_amd import _lib
    n, P = c["n"], c["h1"] * c["w1"]
    cd = torch.from_numpy(np.ascontiguousarray(coords.transpose(0, 2, 1))).to(DEV)
    gd = torch.from_numpy(np.ascontiguousarray(grad.transpose(0, 2, 1))).to(T_DT[dt]).to(DEV)        # [n,rd*rd,P]

    def launch(out):
        rc = _lib.lib().gs_corr_index_backward(_lib.ptr(cd), _lib.ptr(gd), out, n, c["h1"], c["w1"], c["h2"], c["w2"], radius,
                                               GS_DT[dt], _lib.stream_ptr(DEV))
        _lib.check(rc, "corr_index_backward")

    return _twice(n * P * c["h2"] * c["w2"], dt, launch, prefill_zero=True).reshape(n, P, c["h2"], c["w2"])


def forward_paths(c):
    """(label, dtype, radius, level or None, runner(coords)) for every forward path that runs on this case's target map"""
    out = [("pyr f16 planar", "f16", 3, None, lambda xy: run_pyramid(c, xy, "f16", 0)),
           ("pyr f16 nhwc", "f16", 3, None, lambda xy: run_pyramid(c, xy, "f16", 1)),
           ("pyr f16 nhwc slots", "f16", 3, None, lambda xy: run_pyramid(c, xy, "f16", 1, slots=True)),
           ("pyr f32 planar", "f32", 3, None, lambda xy: run_pyramid(c, xy, "f32", 0)),
           ("pyr f32 nhwc", "f32", 3, None, lambda xy: run_pyramid(c, xy, "f32", 1))]
    if c["w2"] % 16 == 0:
        out += [("pyr f16 nhwc tile8", "f16", 3, None, lambda xy: run_pyramid(c, xy, "f16", 1, TILE8)),
                ("pyr f16 nhwc tile8 slots", "f16", 3, None, lambda xy: run_pyramid(c, xy, "f16", 1, TILE8, slots=True))]
    idx = [(dt, 3, l) for dt in ("f16", "f32", "f64") for l in (0, 2)]
    idx += [(dt, r, 0) for dt in ("f32", "f64") for r in (1, 2, 4)] + [("f16", 1, 0)]
    for dt, r, l in idx:
        out.append((f"idx {dt} r={r} level {l}", dt, r, l,
                    lambda xy, dt=dt, r=r, l=l: run_index(c, xy * np.float32(1.0 / (1 << l)), l, dt, r)))
    return out


def _referee(c, dt, radius, level):
    key = ("gpu", dt, radius, level)
    if key not in c:
        levels = c["levels"] if level is None else [c["levels"][level]]
        coords = c["coords"] if level is None else c["coords"] * np.float32(1.0 / (1 << level))
        rkey = ("gpuref", radius, level)
        if rkey not in c:
            c[rkey] = R.lookup_ref(levels, coords, radius)
        c[key] = c[rkey] + (R.lookup_chain(levels, coords, radius, dt),)
    return c[key]


# ------------------------------------------------------------------------------------------------ the forward entries

@pytest.mark.parametrize("name", R.CASES)
def test_lookup_forward_per_element(built_lib, name):
    """every forward path on one case; prints per path the largest |y - ref| / hard_bound and the bit mismatches"""
    c = R.case(name)
    logical = {}
    for label, dt, radius, level, run in forward_paths(c):
        y = run(c["coords"])
        ref, mag, ssum, chain = _referee(c, dt, radius, level)
        assert y.shape == chain.shape and y.dtype == chain.dtype
        mism = ~R.same_bits(y, chain)
        q = R.ratio(y, ref, mag, ssum, dt)
        pinned = np.isfinite(ref) & ~np.isfinite(chain.astype(np.float64))      # an fp16 overflow of the chain: the bits'
        q = np.where(pinned, 0.0, q)
        checked = int(np.isfinite(q).sum())
        print(f"{name} | {label}: largest |y - ref| / bound {np.nanmax(q):.3f} over {checked} finite references, "
              f"{int(mism.sum())} bit mismatches of {y.size}, {int((~np.isfinite(y.astype(np.float64))).sum())} non-finite taps")
        assert not mism.any(), f"{label}: {int(mism.sum())} elements differ from the chain, first at {np.argwhere(mism)[0]}"
        assert np.nanmax(q) <= 1.0, f"{label}: {np.nanmax(q)}"
        if dt != "f16":
            assert np.array_equal(np.isfinite(y), np.isfinite(ref))
        if label.startswith("pyr"):
            logical.setdefault(dt, []).append((label, y))
    for dt, runs in logical.items():                     # planar, channels_last, tile8 and slots: one logical tensor
        for label, y in runs[1:]:
            assert R.same_bits(y, runs[0][1]).all(), f"{label} != {runs[0][0]}"


# ------------------------------------------------------------------------------------------------ non-finite coordinates

BAD_VALUES = (np.inf, -np.inf, np.nan)                 # one per edge
BAD_PIXELS = lambda P: (0, P - 1, 11)                  # first, last, the middle of the second 8-pixel group


def _ibits(a):
    return np.ascontiguousarray(a).view(np.dtype(f"i{a.itemsize}"))


def _poisoned(c, rot):
    """coords with edge e's BAD_VALUES[e] at the three BAD_PIXELS, in x, in y or in both (rotated by `rot`)"""
    xy = c["coords"].copy()
    P = xy.shape[1]
    for e, v in enumerate(BAD_VALUES):
        for m, p in enumerate(BAD_PIXELS(P)):
            axes = ((0,), (1,), (0, 1))[(m + rot) % 3]
            for a in axes:
                xy[e, p, a] = v
    return xy


@pytest.mark.parametrize("name", [f"{h}x{w}-plain" for h, w in R.TARGETS])
def test_non_finite_coordinates_give_nan_in_every_tap(built_lib, name):
    """inf, -inf and nan, in x, in y and in both, on the first pixel, the last pixel and pixel 11: on every forward path
    that pixel's taps are NaN on every level, and every other element keeps the bits of the run without them"""
    c = R.case(name)
    P = c["h1"] * c["w1"]
    bad = np.zeros((c["n"], P), dtype=bool)
    bad[:, list(BAD_PIXELS(P))] = True
    counted = 0
    for label, dt, radius, level, run in forward_paths(c):
        clean = run(c["coords"])
        assert np.isfinite(clean).all()
        for rot in range(3):
            y = run(_poisoned(c, rot))
            assert np.isnan(y[bad]).all(), f"{label} rot {rot}: {int((~np.isnan(y[bad])).sum())} taps of a bad pixel are not NaN"
            assert np.array_equal(_ibits(y[~bad]), _ibits(clean[~bad])), f"{label} rot {rot}: another pixel changed"
            counted += int(bad.sum()) * y.shape[-1]
    print(f"{name}: {counted} taps of pixels with a non-finite coordinate are NaN")


@pytest.mark.parametrize("name", [f"{h}x{w}-plain" for h, w in R.TARGETS])
@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("radius", [3, 2])
def test_lookup_backward_is_the_float64_adjoint(built_lib, name, dt, radius):
    """gs_corr_index_backward per element against lookup_referee.backward_ref (each cell: at most 4 products and 4 sums,
    |B - ref| <= 8 u B(|G|) (1 + 2^-9) + 8 tiny, exactly 0 where nothing lands), and the adjoint identity <F(V), G> =
    <V, B(G)> per pixel in float64 with random V to 8 u sum |V| B(|G|) -- B(|G|) from the float64 model.  The slices of
    pixels whose window lies wholly outside the map stay exactly zero, and so do those of pixels with a non-finite
    coordinate (on the poisoned coordinates of the test above), where every other slice keeps its bits."""
    c = R.case(name)
    n, P, rd = c["n"], c["h1"] * c["w1"], 2 * radius + 1
    rng = np.random.default_rng(77 + rd)
    G = rng.standard_normal((n, P, rd * rd)).astype(R.NP_DT[dt])
    V = rng.standard_normal((n, P, c["h2"], c["w2"]))
    u, tiny = (2.0 ** -24, 2.0 ** -149) if dt == "f32" else (2.0 ** -53, 2.0 ** -1074)
    B = run_backward(c, c["coords"], G, dt, radius).astype(np.float64)
    ref, babs = R.backward_ref(c["coords"], G.astype(np.float64), radius, c["h2"], c["w2"])
    bound = 8.0 * u * babs * (1.0 + 2.0 ** -9) + 8.0 * tiny * (babs > 0)
    err = np.abs(B - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0.0, 0.0, err / bound)
    fwd, mag, _ = R.lookup_ref([V], c["coords"], radius)
    Gd = G.astype(np.longdouble)
    lhs = (fwd.astype(np.longdouble) * Gd).sum(-1)
    rhs = (V.astype(np.longdouble) * B.astype(np.longdouble)).sum((-1, -2))
    scale = (np.abs(V) * babs).sum((-1, -2))
    with np.errstate(divide="ignore", invalid="ignore"):
        qa = np.where(lhs == rhs, 0.0, np.abs(lhs - rhs).astype(np.float64) / (8.0 * u * scale))
    outside = babs.sum((-1, -2)) == 0
    print(f"{name} | backward {dt} r={radius}: largest |B - ref| / bound {q.max():.3f}, adjoint identity {qa.max():.3f} of its "
          f"bound, {int(outside.sum())} slices wholly outside")
    assert q.max() <= 1.0 and qa.max() <= 1.0
    assert outside.any() and not B[outside].any()
    bad = np.zeros((n, P), dtype=bool)
    bad[:, list(BAD_PIXELS(P))] = True
    for rot in range(3):
        Bp = run_backward(c, _poisoned(c, rot), G, dt, radius)
        assert not Bp[bad].any(), "a pixel with a non-finite coordinate wrote to its slice"
        assert np.array_equal(Bp[~bad].astype(np.float64), B[~bad])
