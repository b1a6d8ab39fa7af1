"""The update step's kernels that reduce over pixels or edges, per element against tests/pool_referee.py.

gs_gru_glo and gs_gru_glo_fused (ConvGRU global context), gs_segment_mean (GraphAgg's scatter-mean), gs_bias_act (all six
instantiations over every fp16 bit pattern) and the index-list / persistent-loop paths of gs_cvx_upsample and
gs_upmask_upsample.  The referee evaluates each kernel's documented rounding chain on the CPU in float64 from the very
operands the kernel reads and gives, per output element, the set of admissible fp16 values -- one value wherever the
chain is exact or the fp32 error bound stays clear of an fp16 rounding boundary; tests/test_pool_referee_cpu.py shows
that a lost, doubled or clamped-and-counted pixel, a missing fp16 rounding, an fp16 accumulator and a wrong divisor all
fail it.  The upsampling kernels are judged by test_epilogue_numerics_gpu._cvx_reference on a mask that is known exactly.
Nothing computed on the GPU acts as referee.

Every kernel is called through ctypes; every output lies between two guard regions and is prefilled, like them, with a
NaN of a bit pattern no kernel produces: every element must be overwritten, the guards must keep the pattern.  Every call
runs twice and must give the same bits.

The seeded random sets and the exact regime keep >= 95 % of the pooled means at ONE admissible value (asserted on the CPU
for these very inputs); the fused path's random set therefore keeps W and net on a 1/64 grid, where the matrix-core sum
is exact in any order (pool_referee.glo_conv_weight).  Outside that condition and judged all the same: the extra cases
(zero-mean net; W and net off the grid) and the edge values.

MEASURED (MI355X; per path over all runs of this file; "single" = share of outputs with one admissible value; the ratio
is the largest |y - ref| / bound where a bound is used):
  path                          runs   elements     single  mismatches  ratio
  gs_gru_glo heads                14      12288     0.8867           0
  gs_gru_glo mean                  7       2048     0.9927           0
  gs_gru_glo_fused heads          23     608640     0.9310           0
  gs_gru_glo_fused mean           12     199808     0.9886           0
  gs_gru_glo_fused exact heads     6       4608     0.9353           0
  gs_gru_glo_fused exact mean      6       1536     0.9935           0
  glo extra cases heads            3       2304     0.7726           0
  glo extra cases mean             3        768     0.8255           0
  glo impulses heads             362     278016     1.0000           0
  glo impulses mean              362      92672     1.0000           0
  glo edge values heads            2       2304     0.7231           0
  gs_segment_mean                 56     478976          -           0  0.333
  gs_bias_act none / relu         24    1572864          -           0
  gs_bias_act sigmoid             12     786432          -           0         bit-equal 0.99989 .. 1.0
  gs_upmask_upsample               2    1082880          -           0  0.998
  gs_cvx_upsample                  2     326784          -           0  0.997
  upsampling borders              24       6528          -           0  0.001
  ("heads" = all 384 outputs; with dense random weights a head's value lies near an fp16 boundary more often than a
  pooled mean does, and two neighbours are then admissible.)  Before the fixes that came with this file gs_segment_mean
  missed its chain on 1 to 60 elements of a run (0.1 %): the compiler folded product + conversion of channels 0 and 7 of
  every eight into one rounding, so that a mean exactly between two fp16 values rounded differently there; and both
  ReLUs turned a NaN into 0.  None of these figures is a tolerance: the only thresholds are the referee's own (the sets
  themselves, the 0.999 bit-equal share of the sigmoid, the bound of _cvx_reference)."""
import itertools

import numpy as np
import pytest
import torch

import pool_referee as R
from test_epilogue_numerics_gpu import _cvx_reference

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 256
SENT = {np.float32: (np.int32, 0x7FC0BEEF), np.float16: (np.int16, 0x7E5A)}       # quiet NaNs with a payload
TORCH_INT = {np.int32: torch.int32, np.int16: torch.int16}
f16, f32 = np.float16, np.float32
_TALLY = {}


@pytest.fixture(autouse=True)
def _stop_after_a_device_error():
    """a failed assertion lets the next test run; a device error ends the session (nothing more is launched after it)"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as exc:
        pytest.exit(f"device error, stopping: {exc}", returncode=3)


@pytest.fixture(scope="module", autouse=True)
def _print_tally():
    yield
    print("\npath                          runs   elements     single  mismatches  largest |y - ref| / bound")
    for path, t in _TALLY.items():
        single = f"{t['single'] / t['elements']:.4f}" if t["single"] is not None else "     -"
        ratio = f"{t['ratio']:.3f}" if t["ratio"] is not None else "-"
        print(f"  {path:<28}{t['runs']:>5}{t['elements']:>11}   {single:>8}{t['mismatches']:>12}  {ratio}")


def _tally(path, res, ratio=None):
    t = _TALLY.setdefault(path, {"runs": 0, "elements": 0, "single": None, "mismatches": 0, "ratio": None})
    t["runs"] += 1
    t["elements"] += res["elements"]
    t["mismatches"] += res["mismatches"]
    if "single" in res:
        t["single"] = (t["single"] or 0.0) + res["single"] * res["elements"]
    if ratio is not None:
        t["ratio"] = max(t["ratio"] or 0.0, ratio)
    print(res["line"])
    return res


def _L():
    from go_slam_amd import _lib
    return _lib, _lib.lib(), _lib.stream_ptr(DEV)


def _dev16(a):
    return torch.from_numpy(np.ascontiguousarray(a, f16).view(np.int16)).to(DEV).view(torch.float16)


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, f32)).to(DEV)


def _sentinel(numel, dtype):
    """a device buffer of GUARD + numel + GUARD elements holding the sentinel pattern; -> (whole buffer, the numel body)"""
    it, bits = SENT[dtype]
    whole = torch.full((numel + 2 * GUARD,), bits, dtype=TORCH_INT[it], device=DEV)
    return whole, whole[GUARD:GUARD + numel].view(torch.float32 if dtype is f32 else torch.float16)


def _collect(whole, numel, dtype, what, written=None, exempt=None):
    """the body as numpy; the guards keep the sentinel, every body element (or exactly the `written` mask) lost it.
    exempt: elements whose correct value IS the sentinel's bit pattern (an input NaN with that payload) count as written"""
    it, bits = SENT[dtype]
    raw = whole.cpu().numpy()
    assert (raw[:GUARD] == bits).all() and (raw[GUARD + numel:] == bits).all(), f"{what}: wrote outside the output"
    body = raw[GUARD:GUARD + numel]
    fresh = body != bits
    if exempt is not None:
        fresh = fresh | np.asarray(exempt).reshape(-1)
    if written is None:
        assert fresh.all(), f"{what}: {int((~fresh).sum())} of {numel} elements never written"
    else:
        assert np.array_equal(fresh, np.asarray(written).reshape(-1)), \
            f"{what}: written {int(fresh.sum())}, expected {int(np.sum(written))}"
    return body.view(dtype).copy()


def _twice(once):
    """run a call twice from fresh sentinels: the same bits"""
    a, b = once(), once()
    for u, v in zip(a, b):
        assert np.array_equal(u.view(np.uint8), v.view(np.uint8)), "two runs differ"
    return a


# ------------------------------------------------------------------------------------------------ global context

def _run_glo(net, heads, w_bias, fused, w_pre=None, w=None, stride=128):
    """gs_gru_glo (w_pre) / gs_gru_glo_fused (w) -> (gzr [n,256], gq [n,128]) f32.  The channels past 128 of a wider net
    row are NaN; the workspace starts as NaN bit patterns."""
    from go_slam_amd.droid_net import pack_1x1_weight
    _lib, L, st = _L()
    n, hw = net.shape[:2]
    buf = np.full((n, hw, stride), np.nan, f16)
    buf[..., :128] = net
    d_net, d_b = _dev16(buf), _f32(w_bias)
    hd = [_dev16(h) for h in heads[:3]] + [_f32(h) for h in heads[3:]]
    if fused:
        wp = pack_1x1_weight(torch.from_numpy(w.astype(f32)).view(128, 128, 1, 1).to(DEV))
        nbytes = L.gs_gru_glo_fused_workspace_bytes(n, hw)
    else:
        assert stride == 128
        d_pre = _dev16(w_pre)
        nbytes = L.gs_gru_glo_workspace_bytes(n)

    def once():
        gzr_w, gzr = _sentinel(n * 256, f32)
        gq_w, gq = _sentinel(n * 128, f32)
        ws = torch.full((nbytes,), 255, dtype=torch.uint8, device=DEV)
        if fused:
            rc = L.gs_gru_glo_fused(_lib.ptr(d_net), stride, _lib.ptr(wp), _lib.ptr(d_b), *[_lib.ptr(t) for t in hd],
                                    _lib.ptr(gzr), _lib.ptr(gq), n, hw, _lib.ptr(ws), nbytes, st)
        else:
            rc = L.gs_gru_glo(_lib.ptr(d_pre), _lib.ptr(d_b), _lib.ptr(d_net), *[_lib.ptr(t) for t in hd], _lib.ptr(gzr),
                              _lib.ptr(gq), n, hw, _lib.ptr(ws), nbytes, st)
        _lib.check(rc, "gru_glo_fused" if fused else "gru_glo")
        torch.cuda.synchronize()
        return (_collect(gzr_w, n * 256, f32, "gzr").reshape(n, 256), _collect(gq_w, n * 128, f32, "gq").reshape(n, 128))

    return _twice(once)


def _judge_glo(gzr, gq, ref, path, label, probe):
    bad = _tally(path + " heads", R.judge(np.concatenate([gzr, gq], 1), np.concatenate([ref["gzr"][0], ref["gq"][0]], 1),
                                          np.concatenate([ref["gzr"][1], ref["gq"][1]], 1), label))["mismatches"]
    if probe:                                   # identity on z: the first 128 outputs ARE the pooled mean, bit for bit
        bad += _tally(path + " mean", R.judge(gzr[:, :128], *ref["mean"], label=label + " pooled mean"))["mismatches"]
    assert bad == 0, f"{label}: {bad} outputs outside their admissible sets"


def _run_case(case, fused, stride=128):
    return _run_glo(case["net"], case["heads"], case["w_bias"], fused, w_pre=case.get("w_pre"), w=case.get("w"),
                    stride=stride)


@pytest.mark.parametrize("heads", ["probe", "random"])
@pytest.mark.parametrize("n,hw", R.GLO_SHAPES)
def test_gru_glo_random(built_lib, n, hw, heads):
    case = R.glo_random_case(n, hw, False, heads)
    gzr, gq = _run_case(case, False)
    _judge_glo(gzr, gq, case["ref"], "gs_gru_glo", f"glo ({n}, {hw}) {heads}", heads == "probe")


@pytest.mark.parametrize("heads", ["probe", "random"])
@pytest.mark.parametrize("n,hw,stride", R.FUSED_SHAPES)
def test_gru_glo_fused_random(built_lib, n, hw, stride, heads):
    case = R.glo_random_case(n, hw, True, heads)
    gzr, gq = _run_case(case, True, stride)
    _judge_glo(gzr, gq, case["ref"], "gs_gru_glo_fused", f"glo_fused ({n}, {hw}, {stride}) {heads}", heads == "probe")


def test_gru_glo_fused_block_loop(built_lib):
    """n ceil(hw / 32) = 3074 blocks on 768 workgroups of four waves: the first two waves take a second block"""
    n, hw, stride = R.FUSED_LOOP_SHAPE
    assert n * -(-hw // 32) > 3072
    case = R.glo_random_case(n, hw, True, "probe")
    gzr, gq = _run_case(case, True, stride)
    _judge_glo(gzr, gq, case["ref"], "gs_gru_glo_fused", f"glo_fused ({n}, {hw}) block loop", True)


@pytest.mark.parametrize("fused,extra", [(False, "zero mean"), (True, "zero mean"), (True, "off grid")])
def test_gru_glo_extra_cases(built_lib, fused, extra):
    """zero-mean net (small means against a large sum |t|) and, fused, operands off the 1/64 grid (the matrix-core sum is
    no longer exact): judged like every other set, outside the 95 % condition"""
    case = R.glo_random_case(2, 851, fused, "probe", extra=extra)
    gzr, gq = _run_case(case, fused)
    _judge_glo(gzr, gq, case["ref"], "glo extra cases", f"glo fused={fused} {extra}", True)


@pytest.mark.parametrize("kind", ["identity", "permutation", "dense"])
@pytest.mark.parametrize("n,hw,stride", R.EXACT_SHAPES)
def test_gru_glo_fused_exact_regime(built_lib, n, hw, stride, kind):
    """W, net and the bias are small dyadic numbers: W net + b is exact in fp32 in any order and p is known"""
    w, bias, net = R.glo_exact_inputs(n, hw, 100 + hw, kind)
    heads = R.glo_heads("probe", np.random.default_rng(hw))
    p = R.glo_pre_fused(net, w, bias, exact=True)
    ref = R.glo_referee(p[0], p[1], net, heads, True)
    gzr, gq = _run_glo(net, heads, bias, True, w=w, stride=stride)
    _judge_glo(gzr, gq, ref, "gs_gru_glo_fused exact", f"glo_fused exact {kind} ({n}, {hw})", True)


@pytest.mark.parametrize("hw", [33, 96, 851, 1000])
@pytest.mark.parametrize("fused", [False, True], ids=["two-kernel", "fused"])
def test_gru_glo_impulses(built_lib, fused, hw):
    """g = 1 (w_bias = 30), net = 1024 at ONE pixel of edge 1, edge 0 all zero: the pooled mean is half(1024 fp32(1 / hw))
    on edge 1 and 0 on edge 0 -- a lost or doubled pixel changes it by a factor.  Every set has one value."""
    heads = R.glo_heads("dyadic", np.random.default_rng(3))
    bias = np.full(128, 30.0, f32)
    w = np.abs(R.glo_conv_weight(9)[0])                  # fused: W >= 0, so W net + 30 >= 30 at the impulse too
    want = R.round16(1024.0 * float(f32(1.0) / f32(hw)))
    for pixel in R.impulse_pixels(hw, fused):
        net = R.glo_impulse(2, hw, pixel, 1)
        if fused:
            p = R.glo_pre_fused(net, w, bias, exact=True)
            gzr, gq = _run_glo(net, heads, bias, True, w=w)
        else:
            p = R.glo_pre_two_kernel(np.zeros((2, hw, 128), f16), bias)
            gzr, gq = _run_glo(net, heads, bias, False, w_pre=np.zeros((2, hw, 128), f16))
        ref = R.glo_referee(p[0], p[1], net, heads, fused)
        assert all(R.single(*ref[k]).all() for k in ("mean", "gzr", "gq"))
        assert np.all(ref["mean"][0][1] == want) and np.all(ref["mean"][0][0] == 0.0)
        _judge_glo(gzr, gq, ref, "glo impulses", f"impulse fused={fused} hw={hw} pixel={pixel}", True)


@pytest.mark.parametrize("fused", [False, True], ids=["two-kernel", "fused"])
def test_gru_glo_edge_values(built_lib, fused):
    """pre-activations at +-65504 and +-inf (w_pre; fused: w_bias), net in the fp16 subnormals on eight channels, and one
    NaN pixel in edge 1: exactly the 384 outputs of edge 1 are NaN, edges 0 and 2 are judged as always"""
    n, hw = 3, 96
    rng = np.random.default_rng(40 + fused)
    heads = R.glo_heads("random", rng)
    w_pre, w_bias, net = R.glo_inputs(n, hw, 41 + fused)
    net = net.copy()
    net[:, :, 8:16] = (rng.integers(-1023, 1024, (n, hw, 8)) * 2.0 ** -24).astype(f16)
    net[1, 37, 5] = np.nan
    ext = np.array([65504.0, -65504.0, np.inf, -np.inf])
    if fused:
        w = R.glo_conv_weight(43, grid=False)[0]
        w_bias = w_bias.copy()
        w_bias[[3, 40, 77, 120]] = ext
        p = R.glo_pre_fused(net, w, w_bias)
        gzr, gq = _run_glo(net, heads, w_bias, True, w=w)
    else:
        w_pre = w_pre.copy()
        w_pre.reshape(-1)[rng.permutation(w_pre.size)[:400]] = np.tile(ext, 100).astype(f16)
        p = R.glo_pre_two_kernel(w_pre, w_bias)
        gzr, gq = _run_glo(net, heads, w_bias, False, w_pre=w_pre)
    ref = R.glo_referee(p[0], p[1], net, heads, fused)
    nan = np.isnan(np.concatenate([gzr, gq], 1))
    assert nan[1].all() and not nan[[0, 2]].any(), f"NaN outputs per edge {nan.sum(1).tolist()}, expected [0, 384, 0]"
    assert np.isnan(ref["gq"][0][1]).all() and np.isfinite(ref["mean"][0][[0, 2]]).all()
    assert float(np.abs(ref["mean"][1][0, 8:16]).max()) < 2.0 ** -14, "the subnormal channels' means are subnormal"
    _judge_glo(gzr, gq, ref, "glo edge values", f"glo edge values fused={fused}", False)


# -------------------------------------------------------------------------------------------------- segment mean

N_EDGES = 60
COMBOS = [(False, False), (True, False), (False, True), (True, True)]                        # (bias, ReLU)


def _run_segment_mean(xbuf, c_off, channels, bias, relu, off, edges, hw):
    """gs_segment_mean on channels [c_off, c_off + channels) of xbuf [E, hw, stride] -> fp16 [S, hw, channels]"""
    _lib, L, st = _L()
    d_x, d_off, d_edges = _dev16(xbuf), torch.from_numpy(off).to(DEV), torch.from_numpy(edges).to(DEV)
    d_b = None if bias is None else _f32(bias)
    n_seg, numel = len(off) - 1, (len(off) - 1) * hw * channels

    def once():
        whole, out = _sentinel(numel, f16)
        rc = L.gs_segment_mean(d_x.data_ptr() + 2 * c_off, xbuf.shape[-1], _lib.ptr(d_b), int(relu), _lib.ptr(d_off),
                               _lib.ptr(d_edges), _lib.ptr(out), n_seg, hw, channels, st)
        _lib.check(rc, "segment_mean")
        torch.cuda.synchronize()
        return (_collect(whole, numel, f16, "segment_mean").reshape(n_seg, hw, channels),)

    return _twice(once)[0]


def _judge_segment(y, x, bias, relu, off, edges, label):
    res = R.judge_segment_mean(y, x, bias, relu, off, edges, label)
    _tally("gs_segment_mean", res, res["ratio"])
    assert res["mismatches"] == 0 and res["over"] == 0, res["line"]
    assert np.all(y[np.diff(off) == 0] == 0), "an empty segment is written as zeros"


@pytest.mark.parametrize("channels,stride,c_off", [(8, 8, 0), (64, 64, 0), (128, 128, 0), (64, 256, 64)])
@pytest.mark.parametrize("hw", [1, 5, 35])
def test_segment_mean_random(built_lib, hw, channels, stride, c_off):
    """segment lengths 1 .. 13 (full groups of four followed by a tail of 1, 2 and 3), an empty segment in the middle and
    one at the end, an unsorted list that uses one edge twice and leaves two unused; all four bias / ReLU combinations;
    dense rows and a 64-channel slice at offset 64 of 256-wide rows (the other channels are NaN)"""
    rng = np.random.default_rng(1000 * hw + stride)
    off, edges = R.segment_lists(N_EDGES, rng)
    x = rng.standard_normal((N_EDGES, hw, channels)).astype(f16)
    xbuf = np.full((N_EDGES, hw, stride), np.nan, f16)
    xbuf[..., c_off:c_off + channels] = x
    for with_bias, relu in COMBOS:
        bias = (0.5 * rng.standard_normal(channels)).astype(f32) if with_bias else None
        y = _run_segment_mean(xbuf, c_off, channels, bias, relu, off, edges, hw)
        _judge_segment(y, x, bias, relu, off, edges, f"segment_mean hw={hw} C={channels}/{stride} bias={with_bias} relu={relu}")


@pytest.mark.parametrize("with_bias,relu", COMBOS)
def test_segment_mean_special_values(built_lib, with_bias, relu):
    """(+60000, -60000, 1) in each of the six orders: 1/3 whatever the order in fp32, 0 or 20000 with an fp16 accumulator;
    x + bias past 65504: the fp16 activation is inf and so is the mean; one NaN stays in its (segment, pixel, channel) --
    under the ReLU too, as torch.relu keeps it"""
    hw, c = 5, 8
    rng = np.random.default_rng(7)
    bias = np.zeros(c, f32) if with_bias else None
    x = np.zeros((3, hw, c), f16)
    x[0], x[1], x[2] = 60000.0, -60000.0, 1.0
    orders = list(itertools.permutations(range(3)))
    off = np.arange(0, 19, 3).astype(np.int32)
    edges = np.asarray(orders, np.int32).reshape(-1)
    y = _run_segment_mean(x, 0, c, bias, relu, off, edges, hw)
    _judge_segment(y, x, bias, relu, off, edges, f"segment_mean cancelling triple bias={with_bias} relu={relu}")
    if not relu:
        assert np.all(y == f16(1.0 / 3.0))
    # overflow and NaN on the random lists
    off, edges = R.segment_lists(N_EDGES, rng)
    x = rng.standard_normal((N_EDGES, hw, c)).astype(f16)
    once = [int(e) for e in edges[off[2]:off[3]]]                         # the five edges of segment 2, each used once
    x[once[4], 2, 3] = np.nan                                             # the tail row of a group of four + 1
    big = np.zeros(c, f32)
    if with_bias:
        x[once[0], 1, 6] = 60000.0
        big[6] = 10000.0
    y = _run_segment_mean(x, 0, c, big if with_bias else None, relu, off, edges, hw)
    _judge_segment(y, x, big if with_bias else None, relu, off, edges, f"segment_mean NaN / inf bias={with_bias} relu={relu}")
    want_nan = np.zeros(y.shape, bool)
    want_nan[2, 2, 3] = True
    assert np.array_equal(np.isnan(y), want_nan)
    if with_bias:
        assert np.isposinf(y[2, 1, 6]) and int(np.isinf(y).sum()) == 1


# --------------------------------------------------------------------------------------------- bias + activation

@pytest.mark.parametrize("layout", ["in place", "dense to slice", "slice to dense"])
@pytest.mark.parametrize("act", [0, 1, 2], ids=["none", "relu", "sigmoid"])
def test_bias_act_every_fp16_pattern(built_lib, act, layout):
    """all six instantiations (with and without bias) over every fp16 bit pattern, bias zero, small and 1e4"""
    _lib, L, st = _L()
    x = R.all_fp16_patterns().reshape(-1, 64)
    rows = x.shape[0]
    rng = np.random.default_rng(21)
    xs, xo, ys, yo = {"in place": (64, 0, 64, 0), "dense to slice": (64, 0, 160, 32), "slice to dense": (160, 96, 64, 0)}[layout]
    xbuf = np.full((rows, xs), np.nan, f16)
    xbuf[:, xo:xo + 64] = x
    for kind in ("none", "zero", "small", "1e4"):
        bias = {"none": None, "zero": np.zeros(64, f32), "small": (0.7 * rng.standard_normal(64)).astype(f32),
                "1e4": np.full(64, 1e4, f32)}[kind]
        d_b = None if bias is None else _f32(bias)
        written = np.zeros((rows, ys), bool)
        written[:, yo:yo + 64] = True
        exempt = np.zeros((rows, ys), bool)             # the two input NaNs that are the sentinel itself (quiet or not)
        exempt[:, yo:yo + 64] = (x.view(np.uint16) | 0x0200) == SENT[f16][1]
        assert int(exempt.sum()) == 2

        def once():
            whole, y = _sentinel(rows * ys, f16)
            if layout == "in place":
                y.copy_(_dev16(xbuf).reshape(-1))
                src = y
            else:
                src = _dev16(xbuf)
            rc = L.gs_bias_act(src.data_ptr() + 2 * xo, _lib.ptr(d_b), y.data_ptr() + 2 * yo, rows, 64, xs, ys, act, st)
            _lib.check(rc, "bias_act")
            torch.cuda.synchronize()
            y_all = _collect(whole, rows * ys, f16, "bias_act", written, exempt).reshape(rows, ys)
            return (np.ascontiguousarray(y_all[:, yo:yo + 64]),)

        y = _twice(once)[0]
        res = _tally(f"gs_bias_act act={act}", R.judge_bias_act(y, x, bias, act, f"bias_act act={act} {layout} bias={kind}"))
        assert res["mismatches"] == 0, res["line"]


# ---------------------------------------------------------------------------------------------------- upsampling

def _exact_mask(m, h, w, rng):
    """x, W, b in multiples of 1/64 small enough that W x + b is exact in fp32 in any order: the fp16 mask is known.
    -> x fp16 [m,h,w,128], W fp16 [576,128], b f32 [576], logits fp16 [m,576,h,w]"""
    x = rng.integers(-4, 5, (m, h, w, 128)).astype(f16)
    W = rng.integers(-16, 17, (576, 128)) / 64.0
    b = np.round(rng.uniform(-6, 6, 576) * 64) / 64
    mask = (x.reshape(-1, 128).astype(np.float64) @ W.T + b).astype(f16)
    return x, W.astype(f16), b.astype(f32), np.ascontiguousarray(mask.reshape(m, h, w, 576).transpose(0, 3, 1, 2))


def _run_upsample(entry, m, h, w, n_frames, ix, seed):
    """entry: "upmask" | "nchw" | "nhwc".  -> (out f32 [n_frames,8h,8w] with every selected frame written and every other
    one still the sentinel, ref, extra) for the frames selected"""
    _lib, L, st = _L()
    rng = np.random.default_rng(seed)
    disps = (rng.random((n_frames, h, w)) * 2 + 0.1).astype(f32)
    x, W, b, logits = _exact_mask(m, h, w, rng)
    frames = list(range(m)) if ix is None else ix
    d_ix = None if ix is None else torch.tensor(ix, dtype=torch.int64, device=DEV)
    d_d = _f32(disps)
    if entry == "upmask":
        ops = (_dev16(x), _dev16(W), _f32(b))
    else:
        ops = (_dev16(logits if entry == "nchw" else logits.transpose(0, 2, 3, 1)),)
    numel = n_frames * 64 * h * w
    written = np.zeros((n_frames, 64 * h * w), bool)
    written[frames] = True

    def once():
        whole, out = _sentinel(numel, f32)
        if entry == "upmask":
            rc = L.gs_upmask_upsample(_lib.ptr(ops[0]), 128, _lib.ptr(ops[1]), _lib.ptr(ops[2]), _lib.ptr(d_d), _lib.ptr(d_ix),
                                      _lib.ptr(out), m, h, w, st)
        else:
            rc = L.gs_cvx_upsample(_lib.ptr(d_d), _lib.ptr(ops[0]), _lib.ptr(d_ix), _lib.ptr(out), m, h, w,
                                   int(entry == "nhwc"), st)
        _lib.check(rc, entry)
        torch.cuda.synchronize()
        return (_collect(whole, numel, f32, entry, written).reshape(n_frames, 8 * h, 8 * w),)

    out = _twice(once)[0]
    ref, extra = _cvx_reference(disps[frames], logits)
    return out[frames].astype(np.float64), ref, extra


def _judge_upsample(out, ref, extra, path, label):
    bound = extra + 1e-7 * np.abs(ref)
    ok = np.isfinite(out) & (np.abs(out - ref) <= bound)
    ratio = float(np.where(np.isfinite(out), np.abs(out - ref) / bound, np.inf).max())
    res = {"elements": int(out.size), "mismatches": int((~ok).sum())}
    res["line"] = f"{label}: {out.size} elements, beyond the bound {res['mismatches']}, largest |y - ref| / bound {ratio:.3f}"
    _tally(path, res, ratio)
    assert res["mismatches"] == 0, res["line"]


IX = [5, 0, 3, 6]


@pytest.mark.parametrize("with_ix", [True, False], ids=["index list", "identity"])
def test_upmask_upsample_persistent_loop(built_lib, with_ix):
    """4 x 47 x 45 = 8460 pixels = 265 blocks of 32 on 256 workgroups: nine workgroups take a second block (the prefetched
    rows and the frame index carried across iterations), the last block holds 12 pixels; frames [5, 0, 3, 6] of seven"""
    m, h, w = 4, 47, 45
    assert -(-m * h * w // 32) == 265 and m * h * w % 32 == 12
    out, ref, extra = _run_upsample("upmask", m, h, w, 7 if with_ix else m, IX if with_ix else None, 70)
    _judge_upsample(out, ref, extra, "gs_upmask_upsample", f"upmask_upsample 4x47x45 ix={with_ix}")


@pytest.mark.parametrize("entry", ["nchw", "nhwc"])
def test_cvx_upsample_index_list(built_lib, entry):
    m, h, w = 3, 23, 37
    out, ref, extra = _run_upsample(entry, m, h, w, 7, IX[:m], 71)
    _judge_upsample(out, ref, extra, "gs_cvx_upsample", f"cvx_upsample {entry} 3x23x37 ix={IX[:m]}")


@pytest.mark.parametrize("m,h,w", [(2, 1, 1), (1, 1, 5), (1, 4, 1), (1, 2, 3)])
@pytest.mark.parametrize("entry", ["upmask", "nchw", "nhwc"])
def test_upsample_border_shapes(built_lib, entry, m, h, w):
    """maps of one row, one column, one pixel: every tap outside the map is zero padding"""
    for ix in (None, [2, 0][:m]):
        out, ref, extra = _run_upsample(entry, m, h, w, m if ix is None else 3, ix, 72 + h * w)
        _judge_upsample(out, ref, extra, "upsampling borders", f"{entry} {m}x{h}x{w} ix={ix}")
