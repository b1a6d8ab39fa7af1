"""The gate of gemm_referee can see a wrong kernel: on the CPU, an fp32 accumulation in gs_conv3x3_pp's order passes it,
and three kernels that are subtly wrong -- each of them within today's rtol = atol = 2e-3 of an fp32 convolution in the
image interior -- fail it."""
import functools

import numpy as np
import pytest
import torch

import gemm_referee as R

SHAPES = [(3, 7, 19, 320, 256), (2, 9, 20, 64, 128)]
CASES = [(s, r) for s in SHAPES for r in ("plain", "offset")]


@functools.lru_cache(maxsize=None)
def _case(shape, regime):
    n, h, w, c, o = shape
    x, wt = R.operands(regime, (n, h, w, c), (o, c, 3, 3), 3.0 * c ** 0.5, seed=1000 * n + c + w)
    return (x, wt) + R.conv3x3_ref(x, wt)


@pytest.mark.parametrize("shape,regime", CASES)
def test_offset_regime_cancels_and_the_baseline_is_a_single_rounding(shape, regime):
    x, wt, ref, mag, K, base = _case(shape, regime)
    inner = np.abs(ref[:, 1:-1, 1:-1]) / mag[:, 1:-1, 1:-1]
    print(f"{shape} {regime}: median |ref| / mag in the interior {np.median(inner):.2e}")
    if regime == "offset":
        assert np.median(inner) < 2e-3
    m = R.measure(base, ref, mag, K)
    assert m["hard"] <= 1.0, m
    if regime == "plain":                    # (offset: the result is so small against mag that fp32 itself flips some %)
        assert m["flip"] < 0.01, m


@pytest.mark.parametrize("shape,regime", CASES)
def test_fp32_accumulation_in_the_kernels_order_passes(shape, regime):
    x, wt, ref, mag, K, base = _case(shape, regime)
    y = R.conv3x3_kernel_order(x, wt).half().numpy()
    res = R.gate(y, ref, mag, K, base, label=f"kernel order {shape} {regime}")
    print(res["line"])


@pytest.mark.parametrize("shape,regime", CASES)
@pytest.mark.parametrize("mutant", ["fp16 accumulator after every chunk", "truncating conversion", "seam not padded"])
def test_wrong_kernels_fail(shape, regime, mutant):
    """Each mutant misses the gate; the two systematic roundings miss BOTH statistical gates, with p99.9 excess >= 1.2e-5
    (three orders above an fp32 sum's) and these flip shares:
      truncation: the discarded fraction exceeds half an ulp on half of the elements -> 0.5 (asserted >= 0.48: five
        binomial sigmas at the 23040 elements of the smaller shape); measured 0.499 .. 0.503.
      fp16 accumulator, ten chunks (C = 320): nine roundings before the final one -> >= 0.5; measured 0.56 / 0.86.
      fp16 accumulator, two chunks (C = 64): the rounding after the second chunk IS the final one, so only ONE rounding is
        wrong.  Its error u is uniform in +-1/2 ulp; the final rounding flips when a boundary lies between the sum and the
        sum + u: probability E|u| / ulp = 1/4 while the result is in the accumulator's binade, 1/8 one binade above, more
        below (offset regime: the result is far smaller than the accumulator).  Asserted >= 0.2; measured 0.27 (plain) /
        0.73 (offset).  The 0.5 of the longer chain is not reached here and is not asked for."""
    x, wt, ref, mag, K, base = _case(shape, regime)
    n, h, w, c, o = shape
    if mutant.startswith("fp16"):
        y = R.conv3x3_kernel_order(x, wt, round_chunks=True).half().numpy()
    elif mutant.startswith("trunc"):
        y = R.truncate16(R.conv3x3_kernel_order(x, wt))
    else:
        y = R.conv3x3_kernel_order(x.reshape(1, n * h, w, c), wt).reshape(n, h, w, o).half().numpy()
    k = R.measure(y, ref, mag, K)
    failed = R.failed_assertions(y, ref, mag, K, base)
    print(f"{mutant} {shape} {regime}: fails {sorted(failed)}; flips {k['flip']:.3f}, p99.9 excess {k['p999']:.2e}, "
          f"hard {k['hard']:.3g}")
    assert failed, "the gate does not see this kernel"
    with pytest.raises(AssertionError):
        R.gate(y, ref, mag, K, base)
    if mutant.startswith("seam"):
        assert "hard" in failed and k["hard"] > 100.0
    else:
        assert {"flip", "excess"} <= failed and k["p999"] >= 1.2e-5
        want = 0.48 if mutant.startswith("trunc") else (0.5 if c == 320 else 0.2)
        assert k["flip"] >= want, (k["flip"], want)


def test_truncation_rounds_toward_zero():
    a = torch.tensor([1.0 + 2.0 ** -11, -(1.0 + 2.0 ** -11), 1.0 + 3 * 2.0 ** -11, 70000.0, 2.0 ** -25, 1.5])
    assert R.truncate16(a).astype(np.float64).tolist() == [1.0, -1.0, 1.0 + 2.0 ** -10, 65504.0, 0.0, 1.5]


def test_two_step_rounds_where_the_kernel_does():
    """ref = fn(round16(pre)) in float64; the baseline is fp16(fp32(fn(fp16 pre))): one fp32 operation, then one rounding"""
    pre = np.array([1.0 + 2.0 ** -11 - 1e-9, 1.0 + 2.0 ** -11 + 1e-9, -0.5, 2.0 ** -13])
    b = np.float64(np.float32(0.3))
    ref, base = R.two_step(pre, pre.astype(np.float16), lambda p: np.maximum(p + b, 0.0))
    assert ref.tolist() == [1.0 + b, 1.0 + 2.0 ** -10 + b, 0.0, 2.0 ** -13 + b]
    want = (np.array([1.0, 1.0 + 2.0 ** -10, -0.5, 2.0 ** -13], dtype=np.float32) + np.float32(0.3)).astype(np.float16)
    assert base.dtype == np.float16 and np.array_equal(base, np.maximum(want, np.float16(0)))


@pytest.mark.parametrize("n_out", [128, 64])
@pytest.mark.parametrize("regime", ["plain", "offset"])
def test_two_step_operation_under_the_unchanged_bounds(n_out, regime):
    """conv -> fp16 -> + bias -> ReLU -> fp16 at the shapes of the GPU test (C = 128): an fp32 accumulation in the kernel's
    order passes the gate as it stands, hard bound included, although its intermediate rounding lands on the other
    neighbour than the reference's on some elements; truncating the LAST conversion still misses the flip share and the
    p99.9 excess -- the max excess is blunt here (the baseline's own is ~1e-4 of mag, see gemm_referee)."""
    n, h, w, c = 2, 9, 20, 128
    x, wt = R.operands(regime, (n, h, w, c), (n_out, c, 3, 3), 3.0 * c ** 0.5, seed=310 + n_out)
    b64 = (0.3 * torch.randn(n_out, generator=torch.Generator().manual_seed(311))).double().numpy()
    pre, pmag, K, pbase = R.conv3x3_ref(x, wt)
    ref, base = R.two_step(pre, pbase, lambda p: np.maximum(p + b64, 0.0))
    mag = pmag + np.abs(b64)
    post = torch.relu(R.conv3x3_kernel_order(x, wt).half().double() + torch.from_numpy(b64)).float()
    y = post.half().numpy()
    assert (y.astype(np.float64) != R.round16(ref)).any()              # some intermediate roundings do differ
    res = R.gate(y, ref, mag, K + 1, base, label=f"bias + ReLU model 128->{n_out} {regime}")
    print(res["line"])
    t = R.measure(R.truncate16(post), ref, mag, K + 1)
    print(f"  truncating: flips {t['flip']:.3f}, p99.9 excess {t['p999']:.2e}, max {t['max']:.2e}, hard {t['hard']:.3f}")
    assert {"flip", "excess"} <= R.failed_assertions(R.truncate16(post), ref, mag, K + 1, base)
    assert t["p999"] > R.EXCESS_FACTOR * res["p999_base"] + R.EXCESS_FLOOR


# ---------------------------------------------------------------------------------- encoder and stem convolutions

def _stem_case(regime):
    x, wt = R.operands(regime, (2, 7, 37, 4), (32, 4, 7, 7), 14.0, seed=1247)
    x[..., 3] = 0
    wt[:, 3] = 0
    return x, wt


@pytest.mark.parametrize("regime", ["plain", "offset"])
def test_conv_ref_bias_points_and_a_correct_convolution_passes(regime):
    """conv_ref's baseline is one rounding without bias, two with an fp16 bias (half(half(conv) + b)), one with an fp32
    bias; an fp32 convolution summed in another order (channels-first taps) passes each gate"""
    x, wt = R.operands(regime, (2, 7, 37, 32), (64, 32, 3, 3), 288 ** 0.5, seed=1232)
    b16 = (0.3 * torch.randn(64, generator=torch.Generator().manual_seed(5))).half()
    other = sum(torch.nn.functional.conv2d(x.float().permute(0, 3, 1, 2)[:, c:c + 1], wt.float()[:, c:c + 1], stride=2, padding=1)
                for c in reversed(range(32))).permute(0, 2, 3, 1)
    for bias in (None, b16, b16.float()):
        ref, mag, K, base, slack = R.conv_ref(x, wt, 3, 2, bias, with_slack=True)
        assert ref.shape == (2, 4, 19, 64) and K == 288 + (bias is not None)
        if slack is not None:                                  # the allowance is needed: the baseline is a correct kernel
            print(f"  two-step slack on {float((slack > 0).mean()):.2e} of the elements; without it the baseline is at "
                  f"{R.measure(base, ref, mag, K)['hard']:.2f} of the hard bound")
            assert bias.dtype == torch.float16 and bool((slack > 0).any())
        if bias is None:
            y = other.half()
        elif bias.dtype == torch.float16:
            y = (other.half().float() + bias.float()).half()
        else:
            y = (other + bias).half()
        print(R.gate(y.numpy(), ref, mag, K, base, slack=slack,
                     label=f"3x3 stride 2 {regime} bias {None if bias is None else bias.dtype}")["line"])
    ref16, _, _, base16 = R.conv_ref(x, wt, 3, 2, b16)
    ref32, _, _, base32 = R.conv_ref(x, wt, 3, 2, b16.float())
    assert (base16 != base32).any() and (R.round16(ref16) != R.round16(ref32)).any()      # the bias point matters


@pytest.mark.parametrize("regime", ["plain", "offset"])
@pytest.mark.parametrize("mutant", ["stem drops the border-straddling tap pair", "stride 2 reads the odd pixels"])
def test_wrong_encoder_convolutions_fail(regime, mutant):
    """the stem's k-group is a PAIR of neighbouring taps (kx = 2 g, 2 g + 1) read as two 8-byte loads: a kernel that drops
    the whole pair when one of its pixels lies outside the image loses the in-image tap of the pair in the border columns;
    a stride-2 kernel that samples input pixels 2 o + 1 instead of 2 o shifts the whole output.  Both miss the hard
    bound."""
    if mutant.startswith("stem"):
        x, wt = _stem_case(regime)
        ref, mag, K, base = R.conv_ref(x, wt, 7, 2)
        n, h, w, _ = x.shape
        xp = torch.nn.functional.pad(x.float().permute(0, 3, 1, 2), (3, 3, 3, 3))
        ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        y = torch.zeros(n, 32, ho, wo)
        for g in range(4):
            for kx in (2 * g, 2 * g + 1):
                if kx > 6:
                    continue
                ix = 2 * torch.arange(wo) - 3 + 2 * g                              # input column of the pair's first tap
                keep = ((ix >= 0) & (ix + 1 < w)).float()                          # the pair lies wholly inside the image
                for ky in range(7):
                    patch = xp[:, :, ky:ky + 2 * ho - 1:2, kx:kx + 2 * wo - 1:2]    # [n,4,ho,wo]
                    y += torch.einsum("nchw,oc->nohw", patch, wt.float()[:, :, ky, kx]) * keep
        y = y.permute(0, 2, 3, 1).half().numpy()
    else:
        x, wt = R.operands(regime, (2, 7, 37, 32), (64, 32, 3, 3), 288 ** 0.5, seed=1232)
        ref, mag, K, base = R.conv_ref(x, wt, 3, 2)
        shifted = torch.nn.functional.pad(x.float(), (0, 0, 0, 1, 0, 1))[:, 1:, 1:]            # pixel (y, x) <- (y + 1, x + 1)
        y = torch.nn.functional.conv2d(shifted.permute(0, 3, 1, 2), wt.float(), stride=2, padding=1).permute(0, 2, 3, 1)
        y = y.half().numpy()
    failed = R.failed_assertions(y, ref, mag, K, base)
    k = R.measure(y, ref, mag, K)
    print(f"{mutant} {regime}: fails {sorted(failed)}; flips {k['flip']:.3f}, hard {k['hard']:.3g}")
    assert "hard" in failed and k["hard"] > 100.0
    with pytest.raises(AssertionError):
        R.gate(y, ref, mag, K, base)
    if mutant.startswith("stem"):                      # only the border columns are wrong: the interior is a correct kernel
        inner = np.zeros(ref.shape, dtype=bool)
        inner[:, :, 2:-2] = True
        assert R.measure(y, ref, mag, K, where=inner)["hard"] <= 1.0
