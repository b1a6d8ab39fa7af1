"""The referee of pool_referee can see a wrong kernel: on the CPU, numpy float32 models of gs_gru_glo, gs_gru_glo_fused,
gs_segment_mean and gs_bias_act in the kernels' own summation order pass it, and every planted fault -- each of them
inside today's atol = 2e-3 / rtol = 1e-2 on zero-mean data -- fails it.  Also asserted here, for the very input sets
tests/test_pool_numerics_gpu.py runs: the admissible sets of the pooled mean are single values on at least 95 % of the
outputs (the referee is sharp), and on every output of every impulse case."""
import itertools

import numpy as np
import pytest

import pool_referee as R

f16, f32 = np.float16, np.float32
MODEL_SHAPES = [(3, 1), (2, 7), (2, 33), (3, 96), (2, 851)]


def _glo_judge(gzr, gq, ref, label):
    a, b = R.judge(gzr, *ref["gzr"], label=label + " gzr"), R.judge(gq, *ref["gq"], label=label + " gq")
    print(a["line"])
    print(b["line"])
    return a["mismatches"] + b["mismatches"]


def _model(case, fused, fault=None):
    return R.glo_model(case["net"], case["heads"], fused, w_pre16=case.get("w_pre"), w16=case.get("w"),
                       w_bias=case["w_bias"], fault=fault)


@pytest.mark.parametrize("fused", [False, True], ids=["two-kernel", "fused"])
@pytest.mark.parametrize("heads", ["probe", "random"])
def test_honest_global_context_passes(fused, heads):
    for n, hw in MODEL_SHAPES + [(2, 1000)]:
        case = R.glo_random_case(n, hw, fused, heads)
        gzr, gq = _model(case, fused)
        assert _glo_judge(gzr, gq, case["ref"], f"model ({n}, {hw}) fused={fused} {heads}") == 0
        if heads == "probe":          # identity on z: the first 128 outputs ARE the pooled mean
            assert R.judge(gzr[:, :128], *case["ref"]["mean"])["mismatches"] == 0


def test_honest_fused_exact_regime_passes_with_single_values():
    for kind in ("identity", "permutation", "dense"):
        w, bias, net = R.glo_exact_inputs(2, 33, 5, kind)
        heads = R.glo_heads("probe", np.random.default_rng(6))
        p = R.glo_pre_fused(net, w, bias, exact=True)
        assert np.array_equal(p[0], p[1])
        ref = R.glo_referee(p[0], p[1], net, heads, True)
        gzr, gq = R.glo_model(net, heads, True, w16=w, w_bias=bias)
        assert _glo_judge(gzr, gq, ref, f"exact {kind}") == 0


@pytest.mark.parametrize("fault", R.GLO_FAULTS)
def test_planted_global_context_faults_fail(fault):
    """each fault on the fused model (`live` missing: at hw = 33, where 31 lanes of the second block hold copies of the
    last pixel); the faults that exist on the two-kernel path as well are planted there too"""
    shapes = [(2, 33)] if fault == "clamped lanes counted" else MODEL_SHAPES[1:]
    paths = [True] if fault in ("clamped lanes counted", "pre-activation rounded twice", "padded pixel count") else [True, False]
    for fused in paths:
        bad = 0
        for n, hw in shapes:
            case = R.glo_random_case(n, hw, fused, "probe")
            gzr, gq = _model(case, fused, fault)
            bad += _glo_judge(gzr, gq, case["ref"], f"{fault} ({n}, {hw}) fused={fused}")
        print(f"{fault}, fused={fused}: {bad} outputs outside their admissible sets")
        assert bad > 0, f"the referee does not see: {fault} (fused={fused})"


def _gpu_random_sets():
    sets = [(n, hw, False, k) for n, hw in R.GLO_SHAPES for k in ("probe", "random")]
    sets += [(n, hw, True, k) for n, hw, _ in R.FUSED_SHAPES for k in ("probe", "random")]
    return sets + [R.FUSED_LOOP_SHAPE[:2] + (True, "probe")]


def test_admissible_sets_are_sharp_on_the_gpu_tests_inputs():
    """>= 95 % of the pooled means of every seeded input set have ONE admissible value (a probe of the chain gave 0.988 to
    1.0); the zero-mean extra case is printed only"""
    for n, hw, fused, kind in _gpu_random_sets():
        lo, hi = R.glo_random_case(n, hw, fused, kind)["ref"]["mean"]
        share = float(R.single(lo, hi).mean())
        print(f"({n}, {hw}) fused={fused} {kind}: single {share:.4f}")
        assert share >= 0.95, (n, hw, fused, kind, share)
    for (n, hw, _), kind in itertools.product(R.EXACT_SHAPES, ("identity", "permutation", "dense")):
        w, bias, net = R.glo_exact_inputs(n, hw, 100 + hw, kind)
        p = R.glo_pre_fused(net, w, bias, exact=True)
        lo, hi = R.glo_referee(p[0], p[1], net, R.glo_heads("probe", np.random.default_rng(hw)), True)["mean"]
        share = float(R.single(lo, hi).mean())
        print(f"exact regime ({n}, {hw}) {kind}: single {share:.4f}")
        assert share >= 0.95, (n, hw, kind, share)
    for extra in R.GLO_EXTRAS:
        lo, hi = R.glo_random_case(2, 851, True, "probe", extra=extra)["ref"]["mean"]
        print(f"extra case {extra} (2, 851) fused: single {float(R.single(lo, hi).mean()):.4f}")


@pytest.mark.parametrize("fused", [False, True], ids=["two-kernel", "fused"])
def test_every_impulse_case_has_one_admissible_value(fused):
    heads = R.glo_heads("dyadic", np.random.default_rng(3))
    bias = np.full(128, 30.0, f32)
    for hw in (33, 96, 851, 1000):
        for pixel in R.impulse_pixels(hw, fused):
            net = R.glo_impulse(2, hw, pixel, 1)
            if fused:
                p = R.glo_pre_fused(net, np.abs(R.glo_conv_weight(9)[0]), bias, exact=True)
            else:
                p = R.glo_pre_two_kernel(np.zeros((2, hw, 128), f16), bias)
            ref = R.glo_referee(p[0], p[1], net, heads, fused)
            for key in ("mean", "gzr", "gq"):
                assert R.single(*ref[key]).all(), (hw, pixel, key)
            assert np.all(ref["mean"][0][0] == 0.0) and np.all(ref["mean"][0][1] == R.round16(1024.0 * float(f32(1.0) / f32(hw))))


# ------------------------------------------------------------------------------------------------- segment mean

def _segment_case(seed=11, channels=16, hw=5):
    rng = np.random.default_rng(seed)
    off, edges = R.segment_lists(60, rng)
    x = rng.standard_normal((60, hw, channels)).astype(f16)
    bias = (0.5 * rng.standard_normal(channels)).astype(f32)
    return x, bias, off, edges


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("relu", [False, True])
def test_honest_segment_mean_passes(with_bias, relu):
    x, bias, off, edges = _segment_case()
    bias = bias if with_bias else None
    y = R.segment_mean_model(x, bias, relu, off, edges)
    res = R.judge_segment_mean(y, x, bias, relu, off, edges, label=f"model bias={with_bias} relu={relu}")
    print(res["line"])
    assert res["mismatches"] == 0 and res["over"] == 0
    lengths = np.diff(off)
    assert set(lengths) >= {0, 1, 2, 3, 4, 5, 7, 8, 9, 13} and lengths[-1] == 0 and np.all(y[lengths == 0] == 0)


@pytest.mark.parametrize("fault", R.SEGMENT_FAULTS)
def test_planted_segment_mean_faults_fail(fault):
    x, bias, off, edges = _segment_case()
    y = R.segment_mean_model(x, bias, True, off, edges, fault=fault)
    res = R.judge_segment_mean(y, x, bias, True, off, edges, label=fault)
    print(res["line"])
    assert res["mismatches"] > 0, f"the referee does not see: {fault}"


def test_cancelling_triple_is_exact_in_every_order():
    for order in ([0, 1, 2], [0, 2, 1], [2, 0, 1]):
        x = np.array([60000.0, -60000.0, 1.0], f16).reshape(3, 1, 1).repeat(8, 2)
        y = R.segment_mean_chain(x, None, False, np.array([0, 3]), np.array(order))
        assert np.all(y == f16(f32(1.0) * (f32(1.0) / f32(3.0)))), order


# -------------------------------------------------------------------------------------------- bias + activation

def _bias_act_case(bias_kind):
    x = R.all_fp16_patterns().reshape(-1, 64)
    rng = np.random.default_rng(21)
    bias = {"none": None, "zero": np.zeros(64, f32), "small": (0.7 * rng.standard_normal(64)).astype(f32),
            "1e4": np.full(64, 1e4, f32)}[bias_kind]
    return x, bias


@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("bias_kind", ["none", "zero", "small", "1e4"])
def test_honest_bias_act_passes(act, bias_kind):
    x, bias = _bias_act_case(bias_kind)
    res = R.judge_bias_act(R.bias_act_model(x, bias, act), x, bias, act, label=f"model act={act} bias={bias_kind}")
    print(res["line"])
    assert res["mismatches"] == 0


@pytest.mark.parametrize("fault,act", [("sigmoid of the fp16 sum", 2), ("bias at channel % 8", 0), ("bias at channel % 8", 1),
                                       ("bias at channel % 8", 2)])
def test_planted_bias_act_faults_fail(fault, act):
    x, bias = _bias_act_case("small")
    res = R.judge_bias_act(R.bias_act_model(x, bias, act, fault=fault), x, bias, act, label=f"{fault} act={act}")
    print(res["line"])
    assert res["mismatches"] > 0, f"the referee does not see: {fault}"


def test_relu_keeps_nan_and_sigmoid_saturates():
    x = np.array([np.nan, -np.inf, np.inf, -0.0, 65504.0], f16).repeat(8).reshape(5, 8)
    assert np.isnan(R.bias_act_chain(x, None, 1)[0]).all() and np.all(R.bias_act_chain(x, None, 1)[1] == 0)
    s = R.bias_act_chain(x, None, 2)
    assert np.isnan(s[0]).all() and np.all(s[1] == 0.0) and np.all(s[2] == 1.0) and np.all(s[3] == 0.5)
