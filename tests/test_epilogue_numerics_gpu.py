"""The pointwise and statistics arithmetic around the tracker's big kernels, against float64 at the inputs where such
arithmetic goes wrong: the ConvGRU gates (unfused, gru_gates.hip, and fused into the 3x3 convolution, conv3x3_pp.hip)
over every fp16 value in [-12, 12], a log sweep down to the subnormals, +-1e4, +-65504, +-inf and NaN; the InstanceNorm
statistics of both gs_norm_act paths at mean / spread ratios up to 10^3 and on constant channels; the heads' sigmoid and
softplus epilogues across [-100, 100]; the convex upsampling's softmax at logit spreads up to +-200.

Every reference is the kernel's documented formula evaluated in float64 from the very fp16 / fp32 operands the kernel
reads, rounded where the header documents an fp16 rounding point and once at the end (NumPy rounds float64 -> float16
directly).  The bound is one fp16 ulp of the result plus, where the kernel's fp32 arithmetic legitimately adds error,
a term derived in the test's docstring; a bit-equal fraction catches a systematic bias that stays within one ulp."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EPS24 = 2.0 ** -24


def _L():
    from go_slam_amd import _lib
    return _lib, _lib.lib()


def _ulp16(r):
    """spacing of fp16 at |r| (float64 array): 2^(e - 10), e = max(floor(log2 |r|), -14)"""
    a = np.abs(np.where(np.isfinite(r), r, 0.0))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -24)))
    return 2.0 ** (np.maximum(e, -14) - 10)


def _ulps(a16, b16):
    """integer fp16 ulp distance (monotone integer order of the bit patterns)"""
    ai = a16.view(np.int16).astype(np.int64)
    bi = b16.view(np.int16).astype(np.int64)
    ai = np.where(ai < 0, -32768 - ai, ai)
    bi = np.where(bi < 0, -32768 - bi, bi)
    return np.abs(ai - bi)


def _check16(out16, ref64, extra=0.0, equal_frac=0.999, what=""):
    """out16 (fp16 array) within 1 ulp of half(ref64), or within extra + 1.5 ulp(ref) of ref64 where a derived term
    `extra` applies; NaN / +-inf exactly where the reference has them; at least `equal_frac` of the finite elements
    bit-equal to the correctly rounded reference."""
    ref64 = np.asarray(ref64, np.float64)
    extra = np.broadcast_to(np.asarray(extra, np.float64), ref64.shape).reshape(-1)
    ref64 = ref64.reshape(-1)
    out16 = np.asarray(out16, np.float16).reshape(-1)
    r16 = ref64.astype(np.float16)
    nan_r = np.isnan(ref64)
    assert np.array_equal(np.isnan(out16), nan_r), f"{what}: NaN pattern differs ({int(np.isnan(out16).sum())} vs {int(nan_r.sum())})"
    fin = ~nan_r & np.isfinite(r16)
    inf_r = ~nan_r & ~np.isfinite(r16)
    assert np.array_equal(out16[inf_r], r16[inf_r]), f"{what}: infinities differ"
    o, r = out16[fin].astype(np.float64), ref64[fin]
    d = _ulps(out16[fin], r16[fin])
    ok = (d <= 1) | (np.abs(o - r) <= extra[fin] + 1.5 * _ulp16(r))
    if not ok.all():
        i = np.flatnonzero(~ok)[:8]
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.size} beyond the bound; out {o[i]} ref {r[i]} ulps {d[i]}")
    frac = float((d == 0).mean()) if d.size else 1.0
    assert frac >= equal_frac, f"{what}: only {frac:.5f} bit-equal (need {equal_frac})"


def _sigmoid64(a):
    with np.errstate(over="ignore"):
        return np.where(a >= 0, 1.0 / (1.0 + np.exp(-np.abs(a))), np.exp(-np.abs(a)) / (1.0 + np.exp(-np.abs(a))))


def _preact_values():
    """every fp16 value in [-12, 12], a log sweep +-2^-24 .. 2^-3 (the subnormals included), +-1e4, +-65504, +-inf, NaN"""
    pos = np.arange(0, 0x7C00, dtype=np.uint16).view(np.float16)
    grid = pos[pos <= 12].astype(np.float64)
    sweep = 2.0 ** np.linspace(-24, -3, 211)
    ext = np.array([1e4, 65504.0, np.inf])
    v = np.concatenate([grid, -grid[1:], sweep, -sweep, ext, -ext, [np.nan]])
    return v.astype(np.float16)


def _tile(vals, n_elem, rng):
    """vals, repeated and shuffled to fill n_elem slots (every value appears at least once when n_elem >= len)"""
    reps = -(-n_elem // vals.size)
    t = np.tile(vals, reps)
    head, tail = t[:vals.size], rng.permutation(t[vals.size:])
    return np.concatenate([rng.permutation(head), tail])[:n_elem]


def _net_values(shape, rng):
    """net: 0, +-1 and random values"""
    choice = rng.integers(0, 4, size=shape)
    rnd = rng.standard_normal(shape) * 0.7
    return np.select([choice == 0, choice == 1, choice == 2], [0.0, 1.0, -1.0], rnd).astype(np.float16)


def _dev16(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).to(DEV).view(torch.float16)


def _host16(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.float16)


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


# ------------------------------------------------------------------------------------------ GRU gates, unfused ----

@pytest.mark.parametrize("n,with_inp", [(1, False), (3, True), (3, False), (1, True)])
def test_gru_gate_zr_against_float64(built_lib, n, with_inp):
    """gs_gru_gate_zr: z = half(sigmoid(a_z)), hx[:, :128] = half(sigmoid(a_r) * net) with a = zr_pre + inp_pre + bias +
    glo added in fp32 in that order.  Derived extra term: the three fp32 additions round by at most
    2^-24 (|zr_pre| + |inp_pre| + |bias| + |glo|) each, and sigmoid' <= 1/4, so extra = 3/4 2^-24 sum|operands| (times |net|
    for r * net).  hw = 37 * 53 (no tile multiple), ldx = 264 > 256: channels 128.. of hx stay untouched."""
    _lib, L = _L()
    rng = np.random.default_rng(10 + n + 2 * with_inp)
    hw, ldx = 37 * 53, 264
    vals = _preact_values()
    zr = _tile(vals, n * hw * 256, rng).reshape(n, hw, 256)
    bias = (rng.integers(-8, 9, 256) / 16.0).astype(np.float32)
    glo = (rng.integers(-8, 9, (n, 256)) / 8.0).astype(np.float32)
    glo[:, :8] = 0.0
    bias[:8] = 0.0
    inp = (rng.integers(-16, 17, (n, hw, 384)) / 16.0).astype(np.float16) if with_inp else None
    hx = rng.standard_normal((n, hw, ldx)).astype(np.float16)
    hx[:, :, :128] = _net_values((n, hw, 128), rng)
    hx_d = _dev16(hx)
    z_d = torch.empty(n, hw, 128, dtype=torch.float16, device=DEV)
    zr_d, inp_d = _dev16(zr), (_dev16(inp) if with_inp else None)
    b_d, g_d = _f32(bias), _f32(glo)
    _lib.check(L.gs_gru_gate_zr(_lib.ptr(zr_d), _lib.ptr(b_d), _lib.ptr(g_d), _lib.ptr(inp_d), _lib.ptr(hx_d),
                                _lib.ptr(z_d), n, hw, ldx, _lib.stream_ptr(DEV)), "gru_gate_zr")
    torch.cuda.synchronize()
    zi = inp[..., :256].astype(np.float64) if with_inp else 0.0
    ops = [zr.astype(np.float64), zi, bias.astype(np.float64), glo[:, None, :].astype(np.float64)]
    with np.errstate(invalid="ignore"):
        a = ops[0] + ops[1] + ops[2] + ops[3]
        mag = sum(np.abs(o) for o in ops)
    ea = 0.75 * EPS24 * np.where(np.isfinite(mag), mag, 0.0)
    s = _sigmoid64(a)
    _check16(_host16(z_d), s[..., :128], ea[..., :128], what="z")
    net = hx[:, :, :128].astype(np.float64)
    with np.errstate(invalid="ignore"):
        rn = s[..., 128:] * net
    _check16(_host16(hx_d)[..., :128].reshape(n, hw, 128), rn, ea[..., 128:] * np.abs(net), what="r*net")
    assert np.array_equal(_host16(hx_d).reshape(n, hw, ldx)[..., 128:].view(np.int16), hx[..., 128:].view(np.int16))


def _q_reference(qp, qi, bias, glo, z, net):
    """net_out = (1 - z) net + z tanh(a), a = q_pre + inp_pre + bias + glo; returns (ref, extra): extra = z tanh'(a)
    3 2^-24 sum|a operands| (the fp32 additions) + 4 2^-24 ((1 - z)|net| + z|tanh|) (the blend's four fp32 roundings)"""
    ops = [qp.astype(np.float64), qi, bias.astype(np.float64), glo]
    with np.errstate(invalid="ignore"):
        a = ops[0] + ops[1] + ops[2] + ops[3]
        mag = sum(np.abs(o) for o in ops)
    t = np.tanh(a)
    z = z.astype(np.float64)
    net = net.astype(np.float64)
    with np.errstate(invalid="ignore"):
        ref = (1.0 - z) * net + z * t
        extra = (z * (1.0 - t * t) * 3 * EPS24 * np.where(np.isfinite(mag), mag, 0.0)
                 + 4 * EPS24 * ((1.0 - z) * np.abs(net) + z * np.abs(t)))
    return ref, np.where(np.isfinite(extra), extra, 0.0)


@pytest.mark.parametrize("n,with_inp", [(1, False), (3, True), (3, False), (1, True)])
def test_gru_gate_q_against_float64(built_lib, n, with_inp):
    """gs_gru_gate_q over the pre-activation table with z = 1 and net = 0 on a quarter of the elements (net_out is then
    tanh itself and must be within 1 ulp of half(tanh(x)), no extra term: the sum is exact there) and z, net from
    {0, +-1, random} elsewhere; extra term derived in _q_reference."""
    _lib, L = _L()
    rng = np.random.default_rng(20 + n + 2 * with_inp)
    hw = 37 * 53
    qp = _tile(_preact_values(), n * hw * 128, rng).reshape(n, hw, 128)
    bias = (rng.integers(-8, 9, 128) / 16.0).astype(np.float32)
    glo = (rng.integers(-8, 9, (n, 128)) / 8.0).astype(np.float32)
    bias[:32] = 0.0
    glo[:, :32] = 0.0
    inp = (rng.integers(-16, 17, (n, hw, 384)) / 16.0).astype(np.float16) if with_inp else None
    if with_inp:
        inp[..., 256:288] = 0
    z = rng.random((n, hw, 128)).astype(np.float16)
    z[..., ::3] = np.float16(1.0)
    net = _net_values((n, hw, 128), rng)
    net[..., :32] = 0
    z[..., :32] = 1
    out_d = torch.empty(n, hw, 128, dtype=torch.float16, device=DEV)
    qp_d, inp_d, z_d, net_d = _dev16(qp), (_dev16(inp) if with_inp else None), _dev16(z), _dev16(net)
    b_d, g_d = _f32(bias), _f32(glo)
    _lib.check(L.gs_gru_gate_q(_lib.ptr(qp_d), _lib.ptr(b_d), _lib.ptr(g_d), _lib.ptr(inp_d), _lib.ptr(z_d),
                               _lib.ptr(net_d), _lib.ptr(out_d), n, hw, _lib.stream_ptr(DEV)), "gru_gate_q")
    torch.cuda.synchronize()
    qi = inp[..., 256:].astype(np.float64) if with_inp else 0.0
    ref, extra = _q_reference(qp, qi, bias, glo[:, None, :].astype(np.float64), z, net)
    out = _host16(out_d).reshape(n, hw, 128)
    _check16(out, ref, extra, what="net_out")
    # net = 0, z = 1, a = q_pre exactly: net_out == half(tanh(q_pre)) to one ulp, no extra allowance
    _check16(out[..., :32], np.tanh(qp[..., :32].astype(np.float64)), 0.0, what="tanh itself")


# -------------------------------------------------------------------------- GRU gates fused into the convolution ----

def _fused_gru(n, h, w, c_rest, wscale, inp, bias_zr, glo_zr, bias_q, glo_q, net, xr, rng):
    """run gs_conv3x3_gru_zr2 + gs_conv3x3_gru_q and the unfused pair (gs_conv3x3_pp + gs_gru_gate_zr / _q) on the same
    operands; returns (z, rnet, out) of both as fp16 arrays"""
    from go_slam_amd.droid_net import conv3x3_pp_tile_width, pack_conv3x3_weight
    _lib, L = _L()
    st = _lib.stream_ptr(DEV)
    cin = 128 + c_rest
    wzr = (torch.randn(256, cin, 3, 3, generator=torch.Generator().manual_seed(int(rng.integers(1 << 30)))) * wscale)
    wq = (torch.randn(128, cin, 3, 3, generator=torch.Generator().manual_seed(int(rng.integers(1 << 30)))) * wscale)
    wzr_p, wq_p = pack_conv3x3_weight(wzr.half().to(DEV)), pack_conv3x3_weight(wq.half().to(DEV))
    net_d, xr_d, inp_d = _dev16(net), _dev16(xr), _dev16(inp)
    bzr_d, gzr_d, bq_d, gq_d = _f32(bias_zr), _f32(glo_zr), _f32(bias_q), _f32(glo_q)
    hw = h * w
    z1 = torch.empty(n, hw, 128, dtype=torch.float16, device=DEV)
    rn1, out1 = torch.empty_like(z1), torch.empty_like(z1)
    _lib.check(L.gs_conv3x3_gru_zr2(_lib.ptr(net_d), _lib.ptr(xr_d), c_rest, c_rest, _lib.ptr(wzr_p), _lib.ptr(bzr_d),
                                    _lib.ptr(gzr_d), _lib.ptr(inp_d), _lib.ptr(z1), _lib.ptr(rn1), n, h, w, st), "zr2")
    _lib.check(L.gs_conv3x3_gru_q(_lib.ptr(rn1), _lib.ptr(xr_d), c_rest, c_rest, _lib.ptr(wq_p), _lib.ptr(bq_d),
                                  _lib.ptr(gq_d), _lib.ptr(inp_d), _lib.ptr(z1), _lib.ptr(net_d), _lib.ptr(out1), n, h, w,
                                  st), "q")
    # unfused: hx = [net | x_rest], zr_pre = conv(hx), gate_zr (hx[:, :128] <- r * net), q_pre = conv(hx), gate_q
    hx = torch.cat([net_d.view(n, hw, 128), xr_d.view(n, hw, c_rest)], -1).contiguous()
    zr_pre = torch.empty(n, hw, 256, dtype=torch.float16, device=DEV)
    q_pre = torch.empty(n, hw, 128, dtype=torch.float16, device=DEV)
    z2 = torch.empty_like(z1)
    out2 = torch.empty_like(z1)
    tw = conv3x3_pp_tile_width(w)
    _lib.check(L.gs_conv3x3_pp(_lib.ptr(hx), cin, cin, _lib.ptr(wzr_p), tw, _lib.ptr(zr_pre), 256, 256, n, h, w, 0, st),
               "pp zr")
    _lib.check(L.gs_gru_gate_zr(_lib.ptr(zr_pre), _lib.ptr(bzr_d), _lib.ptr(gzr_d), _lib.ptr(inp_d), _lib.ptr(hx),
                                _lib.ptr(z2), n, hw, cin, st), "gate zr")
    _lib.check(L.gs_conv3x3_pp(_lib.ptr(hx), cin, cin, _lib.ptr(wq_p), tw, _lib.ptr(q_pre), 128, 128, n, h, w, 0, st),
               "pp q")
    _lib.check(L.gs_gru_gate_q(_lib.ptr(q_pre), _lib.ptr(bq_d), _lib.ptr(gq_d), _lib.ptr(inp_d), _lib.ptr(z2),
                               _lib.ptr(net_d), _lib.ptr(out2), n, hw, st), "gate q")
    torch.cuda.synchronize()
    rn2 = hx[..., :128]
    return ([_host16(t).reshape(n, hw, 128) for t in (z1, rn1, out1)],
            [_host16(t).reshape(n, hw, 128) for t in (z2, rn2, out2)])


@pytest.mark.parametrize("h,w", [(60, 80), (23, 37)])
def test_fused_gru_epilogues_at_extremes(built_lib, h, w):
    """gs_conv3x3_gru_zr2 / gs_conv3x3_gru_q.  (1) With zero weights the convolution contributes exactly 0, so the
    pre-activations are inp_pre + bias + glo -- inp_pre carries the whole fp16 table (+-inf and NaN included) and glo the
    per-image offsets: z, r * net and net_out against float64 with the bounds of the unfused tests.  (2) With real
    weights and glo offsets of +-30 / +-1e4 (saturated gates) and 0: equal to the unfused pair under the header's
    equivalence (one ulp, on < 1e-4 of the elements)."""
    rng = np.random.default_rng(h * w)
    n, c_rest, hw = 2, 64, h * w
    inp = _tile(_preact_values(), n * hw * 384, rng).reshape(n, hw, 384)
    r_in = inp[..., 128:256]
    r_in[np.isnan(r_in)] = 0      # (a NaN r makes r * net NaN, and the zero-weight convq turns 0 * NaN into NaN around it)
    net = _net_values((n, hw, 128), rng)
    xr = (rng.standard_normal((n, hw, c_rest)) * 0.5).astype(np.float16)
    bias_zr = np.zeros(256, np.float32)
    bias_q = np.zeros(128, np.float32)
    glo_zr = np.zeros((n, 256), np.float32)
    glo_q = np.zeros((n, 128), np.float32)
    glo_zr[1, :128] = 30.0               # image 1: z -> 1, net_out -> tanh(q) (where net stays finite)
    glo_q[1, :64] = 0.5
    fused, _ = _fused_gru(n, h, w, c_rest, 0.0, inp, bias_zr, glo_zr, bias_q, glo_q, net, xr, rng)
    z1, rn1, out1 = fused
    ops_z = inp[..., :128].astype(np.float64) + glo_zr[:, None, :128]
    z_ref = _sigmoid64(ops_z)
    ez = 0.75 * EPS24 * np.where(np.isfinite(ops_z), np.abs(ops_z), 0.0)
    _check16(z1, z_ref, ez, what="fused z")
    with np.errstate(invalid="ignore"):
        a_r = inp[..., 128:256].astype(np.float64) + glo_zr[:, None, 128:]
        rn_ref = _sigmoid64(a_r) * net.astype(np.float64)
    er = 0.75 * EPS24 * np.where(np.isfinite(a_r), np.abs(a_r), 0.0) * np.abs(net.astype(np.float64))
    _check16(rn1, rn_ref, er, what="fused r*net")
    # net_out from the kernel's own z (fp16, checked above) and net; q = tanh(0-conv + inp_q + glo_q)
    ref, extra = _q_reference(np.zeros_like(inp[..., 256:]), inp[..., 256:].astype(np.float64), np.zeros(128, np.float32),
                              glo_q[:, None, :].astype(np.float64), z1, net)
    # (z spans (0, 1) here: the blend's fp32 roundings -- `extra` -- move the final rounding on ~0.2% of the elements)
    _check16(out1, ref, extra, equal_frac=0.99, what="fused net_out")

    # (2) real weights, saturating offsets: fused == unfused
    inp2 = (rng.standard_normal((n, hw, 384)) * 2).astype(np.float16)
    for off in (0.0, 30.0, -30.0, 1e4, -1e4):
        glo_zr = np.full((n, 256), off, np.float32)
        glo_q = np.full((n, 128), off, np.float32)
        glo_zr[0], glo_q[0] = 0.0, 0.0
        bias_zr = (rng.standard_normal(256) * 0.1).astype(np.float32)
        bias_q = (rng.standard_normal(128) * 0.1).astype(np.float32)
        fused, plain = _fused_gru(n, h, w, c_rest, 0.02, inp2, bias_zr, glo_zr, bias_q, glo_q, net, xr, rng)
        for name, a, b in zip(("z", "r*net"), fused[:2], plain[:2]):
            d = _ulps(a.reshape(-1), b.reshape(-1))
            assert int(d.max()) <= 1, (off, name, int(d.max()))
            assert float((d > 0).mean()) < 1e-4 + 2.0 / d.size, (off, name, float((d > 0).mean()))
        # net_out = (1 - z) net + z q cancels: a 1-ulp difference of z (or of q_pre through r * net) is one fp16 ulp of
        # the blend's TERMS, not of the (possibly much smaller) result
        zf, nf = plain[0].astype(np.float64), net.astype(np.float64)
        scale = np.abs((1 - zf) * nf) + np.abs(zf) + 2.0 ** -14
        d = np.abs(fused[2].astype(np.float64) - plain[2].astype(np.float64))
        assert np.all(d <= 2.0 ** -10 * scale), (off, float((d / scale).max()))
        assert float((d > 0).mean()) < 1e-3, (off, float((d > 0).mean()))


# ------------------------------------------------------------------------------------- InstanceNorm statistics ----

def _norm_case(n, h, w, c, k, rng, ratios, spreads, neg_bias):
    """a 1 x 1 (or centre-tap 3 x 3) stride-1 gs_enc_conv whose input channel 0 is constant 1: channel o of the
    output = m_o + s_o * noise, m_o / s_o from `ratios`; returns (x, wpack, stat_bias)"""
    from go_slam_amd.extractor import pack_enc_conv_weight
    c_in = 128 if k == 1 else 32
    x = (rng.standard_normal((n, h, w, c_in))).astype(np.float16)
    x[..., 0] = 1.0
    s = spreads[np.arange(c) % len(spreads)]
    m = ratios[np.arange(c) % len(ratios)] * np.where(s > 0, s, 0.1)
    W = np.zeros((c, c_in, k, k), np.float32)
    ctr = k // 2
    W[:, 0, ctr, ctr] = m
    W[:, 1:, ctr, ctr] = rng.standard_normal((c, c_in - 1)) * (s / np.sqrt(c_in - 1))[:, None]
    wp = pack_enc_conv_weight(torch.from_numpy(W).half().float().to(DEV))
    b = (-m).astype(np.float16) if neg_bias else np.zeros(c, np.float16)
    return x, wp, b


@pytest.mark.parametrize("n,h,w,c,k", [(1, 240, 320, 32, 3), (2, 37, 53, 128, 1), (2, 60, 80, 256, 1),
                                       (1, 23, 37, 32, 3)])
@pytest.mark.parametrize("neg_bias", [False, True])
def test_norm_act_statistics_paths_against_float64(built_lib, n, h, w, c, k, neg_bias):
    """gs_norm_act with the statistics of gs_enc_conv's epilogue (stat_chunks) and with its own statistics pass, both
    against float64 instance_norm of v = half(half(conv) + stat_bias) built from the kernel's own conv output, at
    m_c / s_c from 0 to 10^3, spreads with s^2 << eps and exactly constant channels, stat_bias 0 and -m_c.
    Bound: 1 ulp where |ref| > 1e-2, plus the fp32 statistics: the mean is an fp32 number and the output is
    (v - mean) invstd in fp32 -> extra = (mean_ulps 2^-24 |mean| + 1e-6 std) invstd + 2^-20 |ref|.  mean_ulps = 2 for the
    fused path (one rounding of K + S1 / N from fp64); 4 for the own-statistics path, whose Chan merges round the running
    fp32 mean once per merge (measured 2.5 fp32 ulps at mean / spread 10^3 -- up to 20 fp16 ulps of outputs near 1e-2).
    Bit-equal on >= 97% (fused) / 95% (own statistics) of those elements: the ratio-10^3 channels, where those fp32
    means move many roundings, are an eighth of the channels.  Then relu(skip + relu(norm)): the sum cancels, so a 1-ulp
    difference of the normalised operand is 1 ulp of that operand (2^-9 relative bound as test_widen_gpu's)."""
    _lib, L = _L()
    st = _lib.stream_ptr(DEV)
    rng = np.random.default_rng(n * h * w + c + neg_bias)
    ratios = np.array([0.0, 1.0, 10.0, 60.0, 100.0, 300.0, 1000.0, 3.0])
    spreads = np.array([0.1, 1.0, 0.1, 0.05, 0.1, 0.03, 0.1, 1e-4, 0.0, 0.5, 1e-3, 0.0, 2.0])
    x, wp, b = _norm_case(n, h, w, c, k, rng, ratios, spreads, neg_bias)
    x_d, b_d = _dev16(x), _dev16(b)
    hw = h * w
    y = torch.empty(n, hw, c, dtype=torch.float16, device=DEV)
    chunks = int(L.gs_enc_conv_stat_chunks(h, w, c))
    nb = int(L.gs_norm_act_workspace_bytes_chunks(n, chunks, c))
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    c_in = x.shape[-1]
    _lib.check(L.gs_enc_conv(_lib.ptr(x_d), c_in, c_in, _lib.ptr(wp), None, _lib.ptr(y), c, c, k, 1, n, h, w,
                             _lib.ptr(b_d), _lib.ptr(ws), st), "enc_conv")
    skip = (rng.standard_normal((n, hw, c))).astype(np.float16)
    skip_d = _dev16(skip)
    out_f = torch.empty_like(y)
    out_c = torch.empty_like(y)
    tail_f = torch.empty_like(y)
    _lib.check(L.gs_norm_act(_lib.ptr(y), _lib.ptr(b_d), None, _lib.ptr(out_f), n, hw, c, 1, 0, 0, 1e-5, _lib.ptr(ws), nb,
                             chunks, st), "norm_act fused")
    _lib.check(L.gs_norm_act(_lib.ptr(y), _lib.ptr(b_d), _lib.ptr(skip_d), _lib.ptr(tail_f), n, hw, c, 1, 1, 1, 1e-5,
                             _lib.ptr(ws), nb, chunks, st), "norm_act fused tail")
    nb2 = int(L.gs_norm_act_workspace_bytes(n, hw, c))
    ws2 = torch.empty(nb2, dtype=torch.uint8, device=DEV)
    _lib.check(L.gs_norm_act(_lib.ptr(y), _lib.ptr(b_d), None, _lib.ptr(out_c), n, hw, c, 1, 0, 0, 1e-5, _lib.ptr(ws2),
                             nb2, 0, st), "norm_act chan")
    torch.cuda.synchronize()
    v = (_host16(y).astype(np.float32) + b.astype(np.float32)).astype(np.float16).reshape(n, hw, c).astype(np.float64)
    mean = v.mean(1, keepdims=True)
    var = v.var(1, keepdims=True)
    inv = 1.0 / np.sqrt(var + 1e-5)
    ref = (v - mean) * inv
    big = np.abs(ref) > 1e-2
    const = (var == 0).reshape(n, 1, c) & np.ones_like(ref, bool)
    for name, out, mean_ulps, frac in (("fused statistics", out_f, 2, 0.97), ("own statistics", out_c, 4, 0.95)):
        extra = (mean_ulps * EPS24 * np.abs(mean) + 1e-6 * np.sqrt(var)) * inv + 2.0 ** -20 * np.abs(ref)
        o = _host16(out).reshape(n, hw, c)
        _check16(o[big], ref[big], np.broadcast_to(extra, ref.shape)[big], equal_frac=frac, what=name)
        assert np.all(o[const] == 0), f"{name}: constant channels must normalise to exactly 0"
        small = ~big & ~const
        assert np.all(np.abs(o[small].astype(np.float64) - ref[small]) <= 2.0 ** -17 + np.broadcast_to(extra, ref.shape)[small]), name
    r16 = np.maximum(ref, 0).astype(np.float16)
    tail_ref = np.maximum(skip.astype(np.float64) + r16.astype(np.float64), 0)
    t = _host16(tail_f).reshape(n, hw, c).astype(np.float64)
    extra = (2 * EPS24 * np.abs(mean) + 1e-6 * np.sqrt(var)) * inv + 2.0 ** -20 * np.abs(ref)
    tol = 2.0 ** -9 * (np.abs(skip.astype(np.float64)) + np.abs(r16.astype(np.float64))) + 1e-6 + extra
    assert np.all(np.abs(t - tail_ref) <= tol), "relu(skip + relu(norm)) tail"


# ------------------------------------------------------------------------------------------------------ heads ----

@pytest.mark.parametrize("n_out", [1, 2])
def test_conv3x3_head_sigmoid_softplus_against_float64(built_lib, n_out):
    """gs_conv3x3_head's epilogues on the kernel's own fp16 pre-activation u = half(conv + bias) (epilogue 0 with
    out_scale 1 returns it exactly), driven across [-100, 100] by weight scale and bias: sigmoid = half(sigmoid(u)) to 1
    ulp; softplus = u for u > 20, log1p(e^u) below, in fp32.  Softplus bound: __expf(u) is exp2(u log2 e) with the
    product rounded (relative error |u| log2(e) ln(2) 2^-24 = |u| 2^-24) plus ~2 ulps of v_exp, and an error eps of
    e^u moves log1p(e^u) by sigmoid(u) eps; log1pf and the final rounding add ~4 ulps of the result:
    |err| <= 2^-24 (sigmoid(u) (2 |u| + 8) + 4 |ref|) (measured: up to 1.7 |u| ulps near u = -85, where e^u nears the
    fp32 subnormals).  The threshold misplaced to 10 errs by log1p(e^-u) = e^-u there, above that bound for u in
    (10, ~12]: caught."""
    from go_slam_amd.droid_net import pack_head_weight
    _lib, L = _L()
    st = _lib.stream_ptr(DEV)
    rng = np.random.default_rng(40 + n_out)
    n, h, w = 2, 37, 53
    x = (rng.standard_normal((n, h, w, 128)) * 1.0).astype(np.float16)
    x_d = _dev16(x)
    res = {}
    for wscale, bias in ((3.0, 0.0), (1.0, 11.0), (1.0, 15.0), (0.3, 19.5), (0.3, 20.5), (6.0, -20.0), (30.0, 0.0),
                         (10.0, 60.0), (10.0, -60.0)):
        wt = torch.from_numpy(rng.standard_normal((n_out, 128, 3, 3)) * wscale / np.sqrt(128 * 9)).float()
        wp = pack_head_weight(wt.half().to(DEV))
        bb = _f32(np.full(n_out, bias))
        outs = []
        for epi in (0, 1, 2):
            o = torch.empty(n, h, w, n_out, dtype=torch.float32, device=DEV)
            _lib.check(L.gs_conv3x3_head(_lib.ptr(x_d), 128, None, 0, _lib.ptr(wp), _lib.ptr(bb), n_out, epi, 1.0,
                                         _lib.ptr(o), n, h, w, st), "head")
            outs.append(o)
        torch.cuda.synchronize()
        u, sg, sp = (o.cpu().numpy().astype(np.float64) for o in outs)
        assert np.array_equal(u, u.astype(np.float16).astype(np.float64)), "epilogue 0 returns the fp16 pre-activation"
        _check16(sg.astype(np.float16), _sigmoid64(u), 0.0, what=f"sigmoid {wscale},{bias}")
        assert np.array_equal(sg, sg.astype(np.float16).astype(np.float64)), "the sigmoid is rounded to fp16"
        ref_sp = np.where(u > 20.0, u, np.log1p(np.exp(np.minimum(u, 20.0))))
        err = np.abs(sp - ref_sp)
        bound = EPS24 * (_sigmoid64(u) * (2 * np.abs(u) + 8) + 4 * np.abs(ref_sp)) + 2.0 ** -126   # (fp32 subnormals flush)
        assert np.all(err <= bound), (wscale, bias, float((err / bound).max()))
        res[(wscale, bias)] = u
    us = np.concatenate([r.reshape(-1) for r in res.values()])
    assert us.min() < -60 and us.max() > 60, "the pre-activations must span the range"
    assert ((us > 10) & (us <= 12)).sum() > 100 and ((us > 20) & (us < 22)).sum() > 100 and ((us > 18) & (us <= 20)).sum() > 100


# ----------------------------------------------------------------------------------------------- upsampling ----

def _cvx_reference(disps, logits):
    """out[f, 8y+i, 8x+j] = sum_k half(softmax64(logits[:, k, lane]))_k * disps[f, y+dy_k, x+dx_k] (zero padded), lane = 8i+j;
    extra = sum_k ulp16(w_k) |nb_k| (one fp16 ulp per weight) + 9 2^-24 sum_k |w_k nb_k| (the fp32 sum)"""
    m, _, h, w = logits.shape
    lg = logits.astype(np.float64).reshape(m, 9, 64, h, w)
    mx = lg.max(1, keepdims=True)
    e = np.exp(lg - mx)
    wk = (e / e.sum(1, keepdims=True)).astype(np.float16).astype(np.float64)
    pad = np.pad(disps.astype(np.float64), ((0, 0), (1, 1), (1, 1)))
    nb = np.stack([pad[:, ky:ky + h, kx:kx + w] for ky in range(3) for kx in range(3)], 1)   # [m, 9, h, w]
    prod = wk * nb[:, :, None]
    ref = prod.sum(1)                                                                      # [m, 64, h, w]
    extra = (_ulp16(wk) * np.abs(nb[:, :, None])).sum(1) + 9 * EPS24 * np.abs(prod).sum(1)
    to_img = lambda a: a.reshape(m, 8, 8, h, w).transpose(0, 3, 1, 4, 2).reshape(m, 8 * h, 8 * w)
    return to_img(ref), to_img(extra)


@pytest.mark.parametrize("channels_last", [False, True])
def test_cvx_upsample_softmax_at_extreme_logits(built_lib, channels_last):
    """gs_cvx_upsample at logit spreads up to +-200 (without the max subtraction e^200 overflows fp32), all nine equal,
    and one dominant logit, against float64 softmax . data; extra term derived in _cvx_reference."""
    _lib, L = _L()
    rng = np.random.default_rng(50 + channels_last)
    m, h, w = 3, 23, 37
    disps = (rng.random((m, h, w)) * 2 + 0.1).astype(np.float32)
    lg = np.empty((m, 9, 64, h, w), np.float32)
    lg[0] = rng.uniform(-200, 200, (9, 64, h, w))                          # wide spreads
    lg[1] = rng.standard_normal((1, 64, h, w)) * 50                        # all nine equal
    lg[2] = rng.standard_normal((9, 64, h, w))
    dom = rng.integers(0, 9, (64, h, w))
    np.put_along_axis(lg[2], dom[None], 150.0, 0)                          # one dominant logit
    lg[2, :, :32] += 120.0                                                 # dominant with large common offsets
    logits = lg.reshape(m, 576, h, w).astype(np.float16)
    mask = torch.from_numpy(logits.view(np.int16)).to(DEV).view(torch.float16)
    if channels_last:
        mask = mask.contiguous(memory_format=torch.channels_last)
    d_d = _f32(disps)
    out = torch.zeros(m, 8 * h, 8 * w, dtype=torch.float32, device=DEV)
    _lib.check(L.gs_cvx_upsample(_lib.ptr(d_d), _lib.ptr(mask), None, _lib.ptr(out), m, h, w, int(channels_last),
                                 _lib.stream_ptr(DEV)), "cvx_upsample")
    torch.cuda.synchronize()
    ref, extra = _cvx_reference(disps, logits)
    o = out.cpu().numpy().astype(np.float64)
    assert np.isfinite(o).all()
    assert np.all(np.abs(o - ref) <= extra + 1e-7 * np.abs(ref)), float((np.abs(o - ref) - extra).max())
    assert float((np.abs(o - ref) <= 4 * EPS24 * np.abs(ref)).mean()) > 0.99


def test_upmask_upsample_equals_unfused_at_extreme_logits(built_lib):
    """gs_upmask_upsample (mask = half(W x + b) inside) against gs_conv1x1 + gs_cvx_upsample on the same operands, with
    logits at +-200 spreads, all nine equal (W = 0, one bias for all nine taps) and one dominant tap.  x, W and b are
    multiples of 1/64 small enough that W x + b is exact in fp32 in any order, so both paths see the same fp16 mask:
    the two outputs and float64 softmax . data of that mask agree within the bound of _cvx_reference."""
    from go_slam_amd.droid_net import pack_1x1_weight
    _lib, L = _L()
    st = _lib.stream_ptr(DEV)
    rng = np.random.default_rng(60)
    m, h, w = 2, 23, 37
    disps = (rng.random((m, h, w)) * 2 + 0.1).astype(np.float32)
    x = rng.integers(-4, 5, (m, h, w, 128)).astype(np.float16)
    x_d, d_d = _dev16(x), _f32(disps)
    q = lambda a: np.round(np.asarray(a) * 64) / 64                      # multiples of 1/64: W x + b exact in fp32
    cases = []
    cases.append((rng.integers(-16, 17, (576, 128)) / 64.0, q(rng.uniform(-200, 200, 576))))
    cases.append((np.zeros((576, 128)), q(np.tile(rng.standard_normal(64) * 30, 9))))
    b3 = np.tile(rng.standard_normal(64), 9)
    b3[4 * 64:5 * 64] += 180.0
    cases.append((rng.integers(-4, 5, (576, 128)) / 64.0, q(b3)))
    for W, bias in cases:
        Wt = torch.from_numpy(W).half().to(DEV)
        b_d = _f32(bias)
        out_f = torch.zeros(m, 8 * h, 8 * w, dtype=torch.float32, device=DEV)
        _lib.check(L.gs_upmask_upsample(_lib.ptr(x_d), 128, _lib.ptr(Wt.contiguous()), _lib.ptr(b_d), _lib.ptr(d_d), None,
                                        _lib.ptr(out_f), m, h, w, st), "upmask_upsample")
        mask = torch.empty(m * h * w, 576, dtype=torch.float16, device=DEV)
        wp = pack_1x1_weight(Wt.float().view(576, 128, 1, 1))
        _lib.check(L.gs_conv1x1(_lib.ptr(x_d), 128, 128, _lib.ptr(wp), _lib.ptr(b_d), 0, _lib.ptr(mask), 576, 576,
                                m * h * w, st), "conv1x1")
        out_u = torch.zeros_like(out_f)
        _lib.check(L.gs_cvx_upsample(_lib.ptr(d_d), _lib.ptr(mask), None, _lib.ptr(out_u), m, h, w, 1, st), "cvx")
        torch.cuda.synchronize()
        logits = _host16(mask).reshape(m, h, w, 576).transpose(0, 3, 1, 2)
        x64 = x.reshape(-1, 128).astype(np.float64) @ W.T + bias
        assert np.array_equal(logits.transpose(0, 2, 3, 1).reshape(-1, 576), x64.astype(np.float16)), "mask not exact"
        ref, extra = _cvx_reference(disps, logits)
        for name, t in (("fused", out_f), ("unfused", out_u)):
            o = t.cpu().numpy().astype(np.float64)
            assert np.isfinite(o).all(), name
            assert np.all(np.abs(o - ref) <= extra + 1e-7 * np.abs(ref)), name
        assert float((out_f - out_u).abs().max()) <= float(2 * extra.max() + 2e-7 * np.abs(ref).max())
