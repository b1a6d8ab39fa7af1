"""CPU checks of the frame encoders' normalisation tail (go_slam_amd/csrc/instnorm.hip) through its NumPy restatement
tools/emulate_instnorm.py: the chunked shifted-sum / Chan-merge statistics against float64, and the rounding chain
against torch's op sequence on fp16 tensors.  On hardware: tests/test_widen_gpu.py::test_norm_act_*."""
import importlib.util
import os

import numpy as np
import torch


def _emu():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "emulate_instnorm.py")
    spec = importlib.util.spec_from_file_location("emulate_instnorm", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_chunked_statistics_match_float64():
    E = _emu()
    rng = np.random.default_rng(3)
    for hw, c, loc, scale in ((700, 32, 0.4, 1.7), (300, 64, -3.0, 0.05), (1000, 128, 10.0, 2.0), (257, 32, 0.0, 1e-3)):
        x = (rng.standard_normal((hw, c)) * scale + loc).astype(np.float16)
        mean, invstd = E.image_stats(x)
        x64 = x.astype(np.float64)
        ref_mean = x64.mean(0)
        ref_inv = 1.0 / np.sqrt(x64.var(0) + 1e-5)
        assert np.allclose(mean, ref_mean, rtol=2e-6, atol=2e-6 * max(1.0, abs(loc)))
        assert np.allclose(invstd, ref_inv, rtol=2e-5), (hw, c)       # (a large mean must not cancel the variance away)


def test_rounding_chain_matches_torch_ops_on_half_tensors():
    """relu(skip + relu(instance_norm(x + b))) with every intermediate an fp16 tensor, as ResidualBlock.forward runs it under
    autocast (src/modules/extractor.py:49-57)"""
    import torch.nn.functional as F
    E = _emu()
    g = torch.Generator().manual_seed(11)
    h, w, c = 12, 20, 32
    x = (torch.randn(1, c, h, w, generator=g) * 1.3 + 0.2).half()
    skip = torch.randn(1, c, h, w, generator=g).half()
    bias = (torch.randn(c, generator=g) * 0.5).half()
    xb = (x.float() + bias.float().view(1, c, 1, 1)).half()
    ref = F.relu((skip.float() + F.relu(F.instance_norm(xb.float()).half()).float()).half())
    to_rows = lambda t: t[0].permute(1, 2, 0).reshape(h * w, c).numpy()
    out = E.norm_act(to_rows(x), bias.numpy(), to_rows(skip), True, True, True)
    diff = np.abs(out.astype(np.float32) - to_rows(ref).astype(np.float32))
    tol = 2.0 ** -9 * (np.abs(to_rows(skip).astype(np.float32)) + np.abs(out.astype(np.float32))) + 1e-6
    assert (diff <= tol).all() and (diff > 0).mean() < 0.02
    plain = E.norm_act(to_rows(x), None, to_rows(skip), False, True, True)
    assert np.array_equal(plain, to_rows(F.relu((skip.float() + F.relu(x).float()).half())))


def _fused_case(rng, ho, wo, c, loc, scale, stat_bias):
    """v = half(half(conv) + stat_bias) for a conv output of mean `loc` and spread `scale` per channel"""
    conv = (rng.standard_normal((ho, wo, c)) * scale + loc).astype(np.float16)
    if stat_bias is None:
        return conv, None
    b = stat_bias.astype(np.float16)
    return (conv.astype(np.float32) + b.astype(np.float32)).astype(np.float16), b


def test_fused_epilogue_statistics_match_float64():
    """gs_enc_conv's epilogue statistics (stats_ws) merged by instnorm_final_sums_kernel, restated by
    emulate_instnorm.fused_moments_stats, against float64 -- the table of test_chunked_statistics_match_float64 plus
    mean / spread ratios up to 10^3, with and without a stat_bias that cancels the mean.  Bounds: the mean is an fp32
    number (|mean| 2^-24 of rounding, counted in units of the spread below), and invstd must hold to 2e-5 relative
    (fp16 outputs have 2^-11 relative half-ulps: 2e-5 is 1/25 of one), whatever the ratio."""
    E = _emu()
    rng = np.random.default_rng(5)
    table = [(0.4, 1.7), (-3.0, 0.05), (10.0, 2.0), (0.0, 1e-3),          # test_chunked_statistics_match_float64
             (1.0, 0.1), (10.0, 0.1), (100.0, 0.1), (-30.0, 0.03), (1000.0, 1.0)]
    shapes = ((37, 53, 32), (23, 70, 64), (5, 40, 128), (3, 33, 256))
    for i, (loc, scale) in enumerate(table):
        ho, wo, c = shapes[i % len(shapes)]
        for bias in (None, np.zeros(c), np.full(c, -loc)):
            v, b = _fused_case(rng, ho, wo, c, loc, scale, bias)
            mean, invstd = E.fused_moments_stats(v, b)
            v64 = v.astype(np.float64).reshape(-1, c)
            ref_mean, ref_var = v64.mean(0), v64.var(0)
            ref_inv = 1.0 / np.sqrt(ref_var + 1e-5)
            assert np.all(np.abs(mean - ref_mean) <= 2.0 ** -22 * np.abs(ref_mean) + 1e-4 * np.sqrt(ref_var) + 1e-7), \
                (loc, scale, c)
            assert np.allclose(invstd, ref_inv, rtol=2e-5, atol=0), (loc, scale, c, np.abs(invstd / ref_inv - 1).max())


def test_fused_epilogue_statistics_at_the_stem_map():
    """The largest slab count: conv1's 240 x 320 map, 32 channels (600 workgroups per image), at mean / spread 10^2 --
    where the former sums of d = v - stat_bias (d not centred: its mean is the convolution's own) lost 1.7e-3 of
    invstd (emulate_instnorm.fused_sums_stats, asserted below so that the emulation of the old scheme stays honest)."""
    E = _emu()
    rng = np.random.default_rng(7)
    v, _ = _fused_case(rng, 240, 320, 32, 10.0, 0.1, None)
    v64 = v.astype(np.float64).reshape(-1, 32)
    ref_inv = 1.0 / np.sqrt(v64.var(0) + 1e-5)
    _, inv = E.fused_moments_stats(v)
    assert np.allclose(inv, ref_inv, rtol=2e-5, atol=0)
    _, inv_old = E.fused_sums_stats(v)
    assert np.abs(inv_old / ref_inv - 1).max() > 1e-4


def test_fused_epilogue_statistics_constant_and_tiny_spread():
    """exactly constant channels -> var 0, invstd = 1 / sqrt(eps) exactly as float64 gives it; spreads with
    s^2 << eps must not come out negative or inflated"""
    E = _emu()
    rng = np.random.default_rng(9)
    ho, wo, c = 19, 45, 32
    v = np.empty((ho, wo, c), np.float16)
    v[:] = (rng.standard_normal(c) * 300).astype(np.float16)
    v[..., 16:] = (v[..., 16:].astype(np.float32) + rng.standard_normal((ho, wo, 16)) * 1e-3).astype(np.float16)
    mean, invstd = E.fused_moments_stats(v)
    v64 = v.astype(np.float64).reshape(-1, c)
    ref_inv = 1.0 / np.sqrt(v64.var(0) + 1e-5)
    assert np.array_equal(invstd[:16], np.full(16, np.float32(1.0 / np.sqrt(1e-5))))
    assert np.array_equal(mean[:16], v[0, 0, :16].astype(np.float32))
    assert np.allclose(invstd, ref_inv, rtol=2e-5, atol=0)


def test_chunked_statistics_at_large_ratios():
    """the Chan path of gs_norm_act (no stat_chunks) at the same ratios as the fused path above"""
    E = _emu()
    rng = np.random.default_rng(4)
    for hw, c, loc, scale in ((4000, 32, 100.0, 0.1), (2000, 64, 1000.0, 1.0), (3000, 32, -30.0, 0.03)):
        x = (rng.standard_normal((hw, c)) * scale + loc).astype(np.float16)
        mean, invstd = E.image_stats(x)
        x64 = x.astype(np.float64)
        ref_inv = 1.0 / np.sqrt(x64.var(0) + 1e-5)
        assert np.allclose(invstd, ref_inv, rtol=2e-5, atol=0), (loc, scale, np.abs(invstd / ref_inv - 1).max())
