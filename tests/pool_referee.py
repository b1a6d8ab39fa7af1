"""A float64 referee for the update step's kernels that reduce over pixels or edges (CPU only: numpy).

gs_gru_glo / gs_gru_glo_fused (ConvGRU global context), gs_segment_mean (GraphAgg's scatter-mean) and gs_bias_act, each
judged by its documented rounding chain (include/goslam_hip.h, csrc/gru_gates.hip) evaluated from the very fp16 / fp32
operands the kernel reads.

What the chain makes exact is reproduced and judged bit for bit: the fp16 x fp16 product (exact in fp32), an fp32 sum in
a documented order (gs_segment_mean), x + bias in fp32.  A sum whose order the contract does not fix is judged by
interval propagation; the result for every output element is a SET of admissible fp16 values [lo, hi], almost always one:

  * a value within the fp32 error bound of an fp16 rounding boundary is ambiguous and contributes both neighbours
    (lo = round16(v - err), hi = round16(v + err)); nothing else widens an interval.  The error is the 1-ulp v_exp /
    v_rcp sigmoid (sigmoid_rel_error) or an fp32 sum taken in another order than float64's;
  * an fp32 sum of t_i is off by at most d 2^-24 sum |t_i| (1 + d 2^-24), d = the longest chain of additions the kernel's
    reduction shape allows (glo_depth), not the number of terms.  The matrix core's adder is not documented as
    round-to-nearest: its d = MFMA_DEPTH counts 2^-23 each, as tests/gemm_referee.py does.

The sign of a zero is not judged.  The second half of the module holds CPU models of the kernels in numpy float32 --
the honest chains and planted faults -- for tests/test_pool_referee_cpu.py."""
import numpy as np

EPS24 = 2.0 ** -24
GLO_CHUNKS = 32                 # gs_gru_glo: pixel chunks per edge
MFMA_DEPTH = 16 + 8             # w(net), K = 128: 16 products inside one MFMA step, 8 steps through the accumulator
f16, f32, f64 = np.float16, np.float32, np.float64


def round16(a):
    """float64 -> the nearest fp16 (one rounding; overflow gives +-inf), returned as float64"""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(a, dtype=f64).astype(f16).astype(f64)


def ulp16(r):
    """spacing of fp16 at |r|: 2^(max(floor(log2 |r|), -14) - 10); non-finite r counts as 0"""
    a = np.abs(np.where(np.isfinite(r), r, 0.0))
    return np.exp2(np.floor(np.log2(np.maximum(a, 2.0 ** -14))) - 10.0)


def sigmoid64(a):
    a = np.asarray(a, f64)
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(-np.abs(a))
        return np.where(np.isnan(a), np.nan, np.where(a >= 0, 1.0 / (1.0 + e), e / (1.0 + e)))


def relu_keep_nan(f):
    """torch.relu: a NaN stays, everything not above zero (-0 included) becomes +0"""
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(f) | (f > 0), f, np.zeros_like(f))


def sigmoid_rel_error(p):
    """relative error bound of gs_sigmoid(p) = v_rcp(1 + v_exp(-p log2 e)) in fp32: the product p log2 e is rounded
    (and log2 e itself is), which moves e^-p by <= 1.5 |p| 2^-24; v_exp 1 ulp (2 2^-24), the addition 2^-24, v_rcp 1 ulp
    (2 2^-24).  Taken as (2 |p| + 8) 2^-24; beyond |p| = 128 the fp32 result is exactly 0 or 1."""
    with np.errstate(invalid="ignore"):
        return (2.0 * np.minimum(np.abs(p), 128.0) + 8.0) * EPS24


def admissible(y, lo, hi):
    """per element: y is an fp16 value inside [lo, hi]; NaN exactly where the interval is NaN"""
    y = np.asarray(y, f64)
    nan = np.isnan(lo) | np.isnan(hi)
    with np.errstate(invalid="ignore"):
        ok = (y == round16(y)) & (y >= lo) & (y <= hi)
    return np.where(nan, np.isnan(y), ok)


def single(lo, hi):
    return (lo == hi) | (np.isnan(lo) & np.isnan(hi))


def judge(y, lo, hi, label=""):
    """-> {elements, single (share of one-element sets), mismatches, line}; nothing is asserted here"""
    ok = admissible(y, lo, hi)
    res = {"elements": int(ok.size), "single": float(single(lo, hi).mean()), "mismatches": int((~ok).sum())}
    res["line"] = f"{label}: {res['elements']} elements, single {res['single']:.4f}, mismatches {res['mismatches']}"
    if res["mismatches"]:
        i = np.flatnonzero(~ok.reshape(-1))[:6]
        res["line"] += (f"; first at {i.tolist()}: got {np.asarray(y, f64).reshape(-1)[i]}, admissible "
                        f"[{np.asarray(lo).reshape(-1)[i]}, {np.asarray(hi).reshape(-1)[i]}]")
    return res


# ---------------------------------------------------------------------------------------------- global context

def glo_depth(hw, fused):
    """the longest chain of fp32 additions between one product and the pooled sum.
    fused (glo_conv_pool_kernel + glo_heads_kernel): 4 rows per lane, 3 butterfly steps, then every third of the
      ceil(hw / 32) block sums one after the other and the 2 additions that join the thirds;
    two kernels (glo_pool_kernel): a chunk holds <= ceil(hw / 32) pixels over 16 lanes, the 16 lane sums one after the
      other, then 32 chunks in thirds (<= 11 each) and the 2 joining additions."""
    blocks = -(-hw // 32)
    if fused:
        return 4 + 3 + -(-blocks // 3) + 2
    return -(-blocks // 16) + 16 + -(-GLO_CHUNKS // 3) + 2


def glo_pre_two_kernel(w_pre16, w_bias):
    """p = half(float(w_pre) + w_bias): exact, so lo = hi"""
    with np.errstate(over="ignore", invalid="ignore"):
        p = (w_pre16.astype(f32) + np.asarray(w_bias, f32)).astype(f16).astype(f64)
    return p, p


def _lsb(a):
    """the largest power of two that divides every (finite, dyadic) element of a"""
    a = np.asarray(a, f64)
    for e in range(16, -40, -1):
        q = 2.0 ** e
        if np.all(a / q == np.round(a / q)):
            return q
    raise AssertionError("operands are not small dyadic numbers")


def glo_pre_fused(net16, w16, w_bias, exact=False):
    """p = half(conv + w_bias), conv = the fp32 matrix-core sum of the 128 products W[o][k] net[k], ONE rounding to fp16.
    exact: W and net are dyadic numbers so small that every partial sum of conv is an fp32 number whatever the order
    (asserted); the fp32 addition of the bias is then the only fp32 rounding and p is known: lo = hi.
    net16 [n,hw,128], w16 [128 out,128 in] -> (lo, hi) [n,hw,128]"""
    x, w, b = net16.astype(f64), w16.astype(f64), np.asarray(w_bias, f64)
    with np.errstate(invalid="ignore", over="ignore"):
        conv = x @ w.T
        mag = np.abs(x) @ np.abs(w).T
        v = conv + b
    if exact:
        assert float(mag.max()) < 2.0 ** 24 * _lsb(w) * _lsb(x), "the exact regime's sums do not fit fp32"
        assert float(np.abs(conv).max()) < 2.0 ** 20 and float(np.abs(b[b != 0]).min(initial=1.0)) > 2.0 ** -20   # v exact in float64
        with np.errstate(over="ignore"):
            p = round16(v.astype(f32).astype(f64))
        return p, p
    with np.errstate(invalid="ignore"):
        err = MFMA_DEPTH * 2.0 ** -23 * (mag + np.abs(b)) + EPS24 * np.abs(v)      # (+ the bias addition's own rounding)
        lo, hi = round16(v - err), round16(v + err)
    return np.where(np.isinf(v), v, lo), np.where(np.isinf(v), v, hi)


def glo_products(p_lo, p_hi, net16):
    """g = half(sigmoid(p)) in [g_lo, g_hi]; t = half(g net) -- the product is exact in fp32, so g determines t"""
    with np.errstate(invalid="ignore"):
        g_lo = round16(sigmoid64(p_lo) * (1.0 - sigmoid_rel_error(p_lo)))
        g_hi = round16(sigmoid64(p_hi) * (1.0 + sigmoid_rel_error(p_hi)))
        x = net16.astype(f64)
        a, b = round16(g_lo * x), round16(g_hi * x)
    return np.minimum(a, b), np.maximum(a, b)


def glo_mean(t_lo, t_hi, hw, depth):
    """half(fp32 sum over the pixels x fp32(1 / hw)); t [n,hw,128] -> (lo, hi) [n,128].  The float64 sums are exact
    (fp16 values are multiples of 2^-24 below 2^16)."""
    assert t_lo.shape[1] == hw
    with np.errstate(invalid="ignore", over="ignore"):
        s_lo, s_hi = t_lo.sum(1), t_hi.sum(1)
        mag = np.maximum(np.abs(t_lo), np.abs(t_hi)).sum(1)
        u = depth * EPS24
        err = u * (1.0 + u) * mag
        inv = f64(f32(1.0) / f32(hw))
        lo, hi = (s_lo - err) * inv, (s_hi + err) * inv
        lo, hi = lo - np.abs(lo) * EPS24, hi + np.abs(hi) * EPS24               # the fp32 multiplication
    return round16(lo), round16(hi)


def glo_head(m_lo, m_hi, w16, bias):
    """half(b + sum_k W[o][k] m[k]): s = b, then s = fmaf(W[o][k], m[k], s) for k = 0 .. 127 -- a documented order, one
    rounding per step, so the error is at most 2^-24 sum_k |s_k| over the partial sums s_k (a tighter form of the
    d = 128 chain's 128 2^-24 sum |t|, times 1 + 128 2^-24 for the second order).  m [n,128] -> (lo, hi) [n,128]"""
    w, b = w16.astype(f64), np.asarray(bias, f64)
    with np.errstate(invalid="ignore", over="ignore"):
        a, c = w[None] * m_lo[:, None, :], w[None] * m_hi[:, None, :]              # [n, out, k]
        s_lo = b[None, :, None] + np.cumsum(np.minimum(a, c), 2)
        s_hi = b[None, :, None] + np.cumsum(np.maximum(a, c), 2)
        # a step whose exact result is an fp32 number rounds nothing: while every step so far was such a one (a zero
        # weight, an identity row, small dyadic operands) the kernel's partial sum IS s_k and the step costs no error
        exact = np.logical_and.accumulate((s_lo == s_hi) & (s_lo == s_lo.astype(f32).astype(f64)), 2)
        step = np.where(exact, 0.0, np.maximum(np.abs(s_lo), np.abs(s_hi)))
        err = EPS24 * (1.0 + 128 * EPS24) * step.sum(2)
        return round16(s_lo[:, :, -1] - err), round16(s_hi[:, :, -1] + err)


def glo_referee(p_lo, p_hi, net16, heads, fused):
    """heads = (wz, wr, wq, bz, br, bq).  -> {"mean": (lo, hi) [n,128], "gzr": (lo, hi) [n,256], "gq": (lo, hi) [n,128]}"""
    hw = net16.shape[1]
    t_lo, t_hi = glo_products(p_lo, p_hi, net16)
    m_lo, m_hi = glo_mean(t_lo, t_hi, hw, glo_depth(hw, fused))
    wz, wr, wq, bz, br, bq = heads
    z, r, q = glo_head(m_lo, m_hi, wz, bz), glo_head(m_lo, m_hi, wr, br), glo_head(m_lo, m_hi, wq, bq)
    return {"mean": (m_lo, m_hi), "gzr": (np.concatenate([z[0], r[0]], 1), np.concatenate([z[1], r[1]], 1)), "gq": q}


def glo_heads(kind, rng):
    """the head sets of the tests.  "probe": identity / zero bias on z (the output IS the pooled mean), a scaled
    permutation on r, random fp16 weights and bias on q; "dyadic": the same with a dyadic q; "random": all three random
    with bias"""
    rnd = lambda: ((rng.standard_normal((128, 128)) / 12.0).astype(f16), (0.3 * rng.standard_normal(128)).astype(f32))
    if kind == "random":
        (wz, bz), (wr, br), (wq, bq) = rnd(), rnd(), rnd()
        return wz, wr, wq, bz, br, bq
    assert kind in ("probe", "dyadic")
    if kind == "dyadic":          # (the impulse cases: q in eighths with a bias in quarters -- its sums are exact in fp32)
        rnd = lambda: ((rng.integers(-4, 5, (128, 128)) / 8.0).astype(f16), (rng.integers(-8, 9, 128) / 4.0).astype(f32))
    wz = np.eye(128, dtype=f16)
    perm = rng.permutation(128)
    while np.array_equal(perm[perm], np.arange(128)):
        perm = rng.permutation(128)
    wr = np.zeros((128, 128), f16)
    wr[np.arange(128), perm] = f16(-1.5)
    wq, bq = rnd()
    return wz, wr, wq, np.zeros(128, f32), np.zeros(128, f32), bq


def glo_inputs(n, hw, seed, zero_mean=False, grid=False):
    """the seeded random set: pre ~ N(0, 2), |net| uniform in [0.25, 1] with one sign per channel (zero_mean: N(0, 0.7),
    small means against a large sum |t| -- an extra case only; grid: net rounded to multiples of 1/64).
    -> w_pre16, w_bias f32, net16, all [n,hw,128] / [128]"""
    rng = np.random.default_rng(seed)
    w_bias = (0.5 * rng.standard_normal(128)).astype(f32)
    w_pre = (2.0 * rng.standard_normal((n, hw, 128)) - w_bias).astype(f16)
    if zero_mean:
        net = 0.7 * rng.standard_normal((n, hw, 128))
    else:
        net = rng.uniform(0.25, 1.0, (n, hw, 128)) * np.where(rng.random(128) < 0.5, -1.0, 1.0)
    if grid:
        net = np.round(net * 64.0) / 64.0
    return w_pre, w_bias, net.astype(f16)


def glo_conv_weight(seed, grid=True):
    """(w fp16 [128,128], w_bias f32) of the fused path's random set: dense N(0, 1/16), bias N(0, 1), so that w(net) + bias
    spreads like N(0, 2).  grid: w in multiples of 1/64 (|w| <= 1); with net on the same grid (|net| <= 4) the products are
    multiples of 2^-12 and sum to less than 2^9 -- the matrix-core sum is exact in ANY order and only the fp32 bias
    (off every grid) rounds.  Without the grid the K = 128 sum's bound, 24 x 2^-23 sum |w net|, makes 9 % of the
    pre-activations ambiguous and the pooled means of few pixels with them (single share 0.89 at hw = 7): that set is
    judged too, but as an extra case outside the 95 % condition."""
    rng = np.random.default_rng(seed)
    w = rng.standard_normal((128, 128)) * 0.25
    if grid:
        w = np.clip(np.round(w * 64.0) / 64.0, -1.0, 1.0)
    return w.astype(f16), rng.standard_normal(128).astype(f32)


def glo_exact_inputs(n, hw, seed, kind):
    """the exact regime of the fused path: net = +-k / 8 (k = 2 .. 8, one sign per channel), W in {identity, permutation,
    dense j / 8 with |j| <= 4}, bias = i / 16: every partial sum of W net + b is a multiple of 2^-6 below 2^7 -- exact in
    fp32 in any order"""
    rng = np.random.default_rng(seed)
    net = (rng.integers(2, 9, (n, hw, 128)) / 8.0 * np.where(rng.random(128) < 0.5, -1.0, 1.0)).astype(f16)
    if kind == "identity":
        w = 2.0 * np.eye(128)
    elif kind == "permutation":
        w = np.zeros((128, 128))
        w[np.arange(128), rng.permutation(128)] = -3.0
    else:
        w = rng.integers(-4, 5, (128, 128)) / 8.0
    bias = (rng.integers(-32, 33, 128) / 16.0).astype(f32)
    return w.astype(f16), bias, net


def glo_impulse(n, hw, pixel, edge, channels=None):
    """net = 0 except 1024 at `pixel` of `edge` (all channels, or `channels`); with w_bias = 30 the gate is exactly 1"""
    net = np.zeros((n, hw, 128), f16)
    net[edge, pixel, slice(None) if channels is None else channels] = 1024.0
    return net


def impulse_pixels(hw, fused):
    """0, 31, 32, hw - 2, hw - 1 and every chunk (two kernels) or 32-pixel block (fused) boundary, inside [0, hw)"""
    if fused:
        edges = [32 * b + d for b in range(-(-hw // 32) + 1) for d in (-1, 0)]
    else:
        edges = [hw * c // GLO_CHUNKS + d for c in range(GLO_CHUNKS + 1) for d in (-1, 0)]
    return sorted({p for p in [0, 31, 32, hw - 2, hw - 1] + edges if 0 <= p < hw})


# (n, hw) of gs_gru_glo: one pixel; fewer pixels than the 16 lanes and most chunks empty; around one 32-pixel block; three
# pixels per chunk; the 23 x 37 map; chunks of 31 and 32 pixels
GLO_SHAPES = [(3, 1), (2, 7), (2, 31), (2, 33), (3, 96), (2, 851), (2, 1000)]
# (n, hw, net_stride) of gs_gru_glo_fused: the same, then ceil(hw / 32) = 29, 30, 31 and 61 (the thirds and the ten-wide
# unrolled sum of glo_heads_kernel: 30 block sums fill one round exactly), then n ceil(hw / 32) = 3074 > 3072 wave slots
# (two blocks per edge, the second one holding a single pixel; as few pixels as such a launch can have)
FUSED_SHAPES = [(n, hw, 136 if i % 2 else 128) for i, (n, hw) in enumerate(GLO_SHAPES)] + \
               [(2, 923, 136), (2, 960, 128), (2, 961, 136), (2, 1951, 128)]
FUSED_LOOP_SHAPE = (1537, 33, 128)
EXACT_SHAPES = [(2, 33, 136), (2, 851, 128)]            # the exact regime's (n, hw, net_stride); seed = 100 + hw
GLO_EXTRAS = ("zero mean", "off grid")
_CASES = {}


def glo_random_case(n, hw, fused, heads_kind, extra=None):
    """the seeded random input set of (n, hw) with its admissible sets, computed once and shared (do not modify):
    {w_pre, w (fused), w_bias, net, heads, ref}.  extra: None, "zero mean" or (fused only) "off grid" -- the two extra
    cases outside the 95 % condition"""
    key = (n, hw, fused, heads_kind, extra)
    if key not in _CASES:
        assert extra in (None, "zero mean", "off grid") and (fused or extra != "off grid")
        seed = 7919 * hw + 31 * n + 2 * int(fused) + (0 if extra is None else len(extra))
        w_pre, w_bias, net = glo_inputs(n, hw, seed, extra == "zero mean", grid=fused and extra != "off grid")
        heads = glo_heads(heads_kind, np.random.default_rng(seed + 1))
        case = {"w_bias": w_bias, "net": net, "heads": heads}
        if fused:
            case["w"], case["w_bias"] = glo_conv_weight(seed + 2, grid=extra != "off grid")
            p = glo_pre_fused(net, case["w"], case["w_bias"], exact=extra != "off grid")
        else:
            case["w_pre"] = w_pre
            p = glo_pre_two_kernel(w_pre, w_bias)
        case["ref"] = glo_referee(p[0], p[1], net, heads, fused)
        _CASES[key] = case
    return _CASES[key]


# ---------------------------------------------------------------------------------------------- segment mean

def segment_act(x16, bias, relu):
    """the operand of the sum as fp32: half(relu?(float(x) + bias)) when a bias or ReLU is given, x otherwise"""
    a = x16.astype(f32)
    if bias is None and not relu:
        return a
    with np.errstate(over="ignore", invalid="ignore"):
        if bias is not None:
            a = a + np.asarray(bias, f32)
        if relu:
            a = relu_keep_nan(a)
        return a.astype(f16).astype(f32)


def segment_mean_chain(x16, bias, relu, offsets, edges):
    """the exact chain in numpy float32: act, a sequential fp32 sum in seg_edges order, x fp32(1 / count), one rounding to
    fp16; an empty segment gives zeros.  x16 [E,hw,C] (the channels the kernel reads) -> fp16 [S,hw,C]"""
    act = segment_act(x16, bias, relu)
    out = np.zeros((len(offsets) - 1,) + x16.shape[1:], f16)
    with np.errstate(over="ignore", invalid="ignore"):
        for s in range(len(offsets) - 1):
            b, e = int(offsets[s]), int(offsets[s + 1])
            if e <= b:
                continue
            acc = np.zeros(x16.shape[1:], f32)
            for k in range(b, e):
                acc = acc + act[int(edges[k])]
            out[s] = (acc * (f32(1.0) / f32(e - b))).astype(f16)
    return out


def segment_mean_float64(x16, bias, relu, offsets, edges):
    """(float64 mean, bound): bound = 1.5 ulp16(mean) + count 2^-24 mean |act|"""
    act = segment_act(x16, bias, relu).astype(f64)
    ref = np.zeros((len(offsets) - 1,) + x16.shape[1:])
    bound = np.full_like(ref, 2.0 ** -30)                         # (an empty segment: any non-zero value is beyond it)
    with np.errstate(over="ignore", invalid="ignore"):
        for s in range(len(offsets) - 1):
            rows = [int(k) for k in edges[int(offsets[s]):int(offsets[s + 1])]]
            if rows:
                ref[s] = act[rows].mean(0)
                bound[s] = 1.5 * ulp16(ref[s]) + len(rows) * EPS24 * np.abs(act[rows]).mean(0)
    return ref, bound


def judge_segment_mean(y16, x16, bias, relu, offsets, edges, label=""):
    """bit for bit against the chain (+-0 alike, NaN where the chain has NaN), and within the bound of the float64 mean
    wherever that is finite (non-finite: the same infinity / NaN).  -> {elements, mismatches, over (elements beyond the
    float64 bound), ratio (largest |y - ref| / bound), line}"""
    want = segment_mean_chain(x16, bias, relu, offsets, edges)
    y = np.asarray(y16, f16)
    yv, wv = y.astype(f64), want.astype(f64)
    same = (yv == wv) | (np.isnan(yv) & np.isnan(wv))
    ref, bound = segment_mean_float64(x16, bias, relu, offsets, edges)
    r16 = round16(ref)
    fin = np.isfinite(r16) & np.isfinite(ref)
    with np.errstate(invalid="ignore"):
        ratio = np.where(fin, np.abs(yv - ref) / np.where(fin, bound, 1.0), 0.0)
        ratio = np.where(fin & ~np.isfinite(yv), np.inf, ratio)
        wild = ~fin & ~((yv == r16) | (np.isnan(yv) & np.isnan(r16)))
    over = int((ratio > 1.0).sum() + wild.sum())
    res = {"elements": int(y.size), "mismatches": int((~same).sum()), "over": over, "ratio": float(ratio.max(initial=0.0))}
    res["line"] = (f"{label}: {res['elements']} elements, mismatches {res['mismatches']}, beyond the float64 bound {over}, "
                   f"largest |y - ref| / bound {res['ratio']:.3f}")
    if res["mismatches"]:
        i = np.argwhere(~same)[:6]
        res["line"] += f"; first at (segment, pixel, channel) {i.tolist()}: got {yv[~same][:6]}, chain {wv[~same][:6]}"
    return res


def segment_lists(n_edges, rng):
    """segment lengths 1, 2, 3, 4, 5, 7, 8, 9, 13 with an empty segment in the middle and one at the end; unsorted,
    edge 0 used in two segments, the last two edges unused.  -> (offsets int32 [S+1], edges int32)"""
    lengths = [4, 1, 5, 0, 2, 8, 3, 13, 7, 9, 0]
    total = sum(lengths)
    assert n_edges >= total + 1
    pool = rng.permutation(n_edges - 2)[:total - 1].tolist()
    edges = pool + [pool[0]]                                     # the last segment's last edge = the first segment's first
    assert len(set(edges)) == total - 1 and edges != sorted(edges)
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32), np.asarray(edges, np.int32)


# ---------------------------------------------------------------------------------------------- bias + activation

def bias_act_chain(x16, bias, act):
    """act 0 / 1: half(relu?(float(x) + bias)), exact.  act 2: (float64 sigmoid of the fp32 sum, None)"""
    with np.errstate(over="ignore", invalid="ignore"):
        a = x16.astype(f32)
        if bias is not None:
            a = a + np.asarray(bias, f32)
        if act == 2:
            return sigmoid64(a.astype(f64))
        if act == 1:
            a = relu_keep_nan(a)
        return a.astype(f16)


def _ulps(a16, b16):
    """integer fp16 ulp distance (monotone integer order of the bit patterns)"""
    ai = a16.view(np.int16).astype(np.int64)
    bi = b16.view(np.int16).astype(np.int64)
    ai = np.where(ai < 0, -32768 - ai, ai)
    bi = np.where(bi < 0, -32768 - bi, bi)
    return np.abs(ai - bi)


def judge_bias_act(y16, x16, bias, act, label="", equal_frac=0.999):
    """act 0 / 1: bit for bit (+-0 alike, NaN where the chain has NaN).  Sigmoid: NaN exactly where the float64 value is
    NaN, within one fp16 ulp of it, and at least `equal_frac` of the elements bit-equal to its correct rounding.
    -> {elements, mismatches, equal (share), line}"""
    y = np.ascontiguousarray(y16, f16)
    want = bias_act_chain(x16, bias, act)
    if act != 2:
        yv, wv = y.astype(f64), want.astype(f64)
        same = (yv == wv) | (np.isnan(yv) & np.isnan(wv))
        res = {"elements": int(y.size), "mismatches": int((~same).sum()), "equal": float(same.mean())}
    else:
        r16 = np.ascontiguousarray(round16(want).astype(f16))
        nan = np.isnan(want)
        d = _ulps(y.reshape(-1), r16.reshape(-1)).reshape(y.shape)
        ok = np.where(nan, np.isnan(y), ~np.isnan(y) & (d <= 1))
        eq = float((d[~nan] == 0).mean()) if (~nan).any() else 1.0
        res = {"elements": int(y.size), "mismatches": int((~ok).sum()) + (0 if eq >= equal_frac else 1), "equal": eq}
    res["line"] = f"{label}: {res['elements']} elements, mismatches {res['mismatches']}, bit-equal {res['equal']:.5f}"
    return res


def all_fp16_patterns():
    return np.arange(1 << 16, dtype=np.uint16).view(f16)


# ---------------------------------------------------------------------------------------------- CPU models of a kernel

def _sigmoid32(p32):
    with np.errstate(over="ignore", invalid="ignore"):
        return (f32(1.0) / (f32(1.0) + np.exp(-p32))).astype(f32)


def _fmaf_head(m32, w16, bias):
    """s = b; s = fmaf(W[o][k], m[k], s) for k = 0 .. 127 (float64 holds product + s up to a double rounding that a model
    may have), then half -> f32 [n,128]"""
    w = w16.astype(f64)
    s = np.broadcast_to(np.asarray(bias, f32), (m32.shape[0], 128)).astype(f32)
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(128):
            s = (s.astype(f64) + w[None, :, k] * m32[:, None, k].astype(f64)).astype(f32)
        return s.astype(f16).astype(f32)


def _thirds(partial):
    """glo_heads_kernel: thread (third, channel) adds every third partial sum in order; (p0 + p1) + p2"""
    part = []
    for third in range(3):
        s = np.zeros(partial.shape[:1] + partial.shape[2:], f32)
        for c in range(third, partial.shape[1], 3):
            s = s + partial[:, c]
        part.append(s)
    return (part[0] + part[1]) + part[2]


def _chunk_partials(t, hw):
    """glo_pool_kernel: chunk c = pixels [hw c / 32, hw (c + 1) / 32), lane l takes every 16th, then the 16 lanes in order"""
    out = np.zeros((t.shape[0], GLO_CHUNKS, 128), f32)
    for c in range(GLO_CHUNKS):
        p0, p1 = hw * c // GLO_CHUNKS, hw * (c + 1) // GLO_CHUNKS
        acc = np.zeros((16, t.shape[0], 128), f32)
        for p in range(p0, p1):
            acc[(p - p0) % 16] = acc[(p - p0) % 16] + t[:, p]
        s = np.zeros((t.shape[0], 128), f32)
        for l in range(16):
            s = s + acc[l]
        out[:, c] = s
    return out


def _block_partials(t, hw, count_clamped):
    """glo_conv_pool_kernel: 32 pixels per block; lane row r adds pixels r, r + 8, r + 16, r + 24, then the xor butterfly
    over the 8 rows.  count_clamped: the out-of-range lanes' copies of pixel hw - 1 are added (`live` missing)"""
    n, blocks = t.shape[0], -(-hw // 32)
    pad = np.zeros((n, blocks * 32, 128), f32)
    pad[:, :hw] = t
    if count_clamped:
        pad[:, hw:] = t[:, hw - 1:hw]
    v = pad.reshape(n, blocks, 4, 8, 128)
    a = ((v[:, :, 0] + v[:, :, 1]) + v[:, :, 2]) + v[:, :, 3]                         # [n, blocks, 8, 128]
    a = a[:, :, 0::2] + a[:, :, 1::2]
    a = a[:, :, 0::2] + a[:, :, 1::2]
    return a[:, :, 0] + a[:, :, 1]


GLO_FAULTS = ("last pixel dropped", "clamped lanes counted", "block dropped", "product not rounded", "sigmoid not rounded",
              "pre-activation rounded twice", "fp16 accumulator", "padded pixel count", "z and r swapped",
              "weight transposed")


def glo_model(net16, heads, fused, w_pre16=None, w16=None, w_bias=None, fault=None):
    """gs_gru_glo (w_pre16) / gs_gru_glo_fused (w16) in numpy float32 in the kernels' summation order -> (gzr f32 [n,256],
    gq f32 [n,128]); fault: None or one of GLO_FAULTS"""
    assert fault is None or fault in GLO_FAULTS
    n, hw = net16.shape[:2]
    x = net16.astype(f32)
    b = np.asarray(w_bias, f32)
    with np.errstate(over="ignore", invalid="ignore"):
        if fused:
            conv = (x.reshape(-1, 128) @ w16.astype(f32).T).reshape(n, hw, 128)
            p = (conv.astype(f16).astype(f32) + b) if fault == "pre-activation rounded twice" else conv + b
        else:
            p = w_pre16.astype(f32) + b
        g = _sigmoid32(p.astype(f16).astype(f32))
        if fault != "sigmoid not rounded":
            g = g.astype(f16).astype(f32)
        t = g * x
        if fault != "product not rounded":
            t = t.astype(f16).astype(f32)
        if fault == "last pixel dropped":
            t = t.copy()
            t[:, hw - 1] = 0.0
        if fault == "fp16 accumulator":
            acc = np.zeros((n, 128), f16)
            for p_ in range(hw):
                acc = acc + t[:, p_].astype(f16)
            s = acc.astype(f32)
        else:
            partial = _block_partials(t, hw, fault == "clamped lanes counted") if fused else _chunk_partials(t, hw)
            if fault == "block dropped":
                partial = partial.copy()
                partial[:, partial.shape[1] // 2] = 0.0
            s = _thirds(partial)
        count = -(-hw // 32) * 32 if fault == "padded pixel count" else hw
        m = (s * (f32(1.0) / f32(count))).astype(f16).astype(f32)
    wz, wr, wq, bz, br, bq = heads
    if fault == "z and r swapped":
        wz, wr, bz, br = wr, wz, br, bz
    if fault == "weight transposed":
        wq = np.ascontiguousarray(wq.T)
    return np.concatenate([_fmaf_head(m, wz, bz), _fmaf_head(m, wr, br)], 1), _fmaf_head(m, wq, bq)


SEGMENT_FAULTS = ("clamped tail row added", "edge e - 1 in every group", "bias after the ReLU", "activation not rounded",
                  "offsets shifted", "count + 1")


def segment_mean_model(x16, bias, relu, offsets, edges, fault=None):
    """segment_mean_kernel in numpy float32: groups of four rows with the tail clamped to e - 1 and skipped"""
    assert fault is None or fault in SEGMENT_FAULTS
    a = x16.astype(f32)
    touch = bias is not None or relu
    with np.errstate(over="ignore", invalid="ignore"):
        if touch:
            bb = np.zeros(x16.shape[-1], f32) if bias is None else np.asarray(bias, f32)
            if fault == "bias after the ReLU":
                a = (relu_keep_nan(a) if relu else a) + bb
            else:
                a = a + bb
                a = relu_keep_nan(a) if relu else a
            if fault != "activation not rounded":
                a = a.astype(f16).astype(f32)
        off = np.asarray(offsets).astype(np.int64)
        if fault == "offsets shifted":
            off = np.concatenate([off[1:], off[-1:]])
        out = np.zeros((len(off) - 1,) + x16.shape[1:], f16)
        for s in range(len(off) - 1):
            b, e = int(off[s]), int(off[s + 1])
            acc = np.zeros(x16.shape[1:], f32)
            for k0 in range(b, e, 4):
                for u in range(4):
                    k = min(k0 + u, e - 1)
                    if k0 + u >= e and not (fault == "clamped tail row added" and k0 + u == e):
                        continue
                    acc = acc + a[int(edges[k])]
                if fault == "edge e - 1 in every group" and k0 + 4 < e:
                    acc = acc + a[int(edges[e - 1])]
            cnt = e - b + (1 if fault == "count + 1" else 0)
            inv = f32(1.0) / f32(cnt) if e > b else f32(0.0)
            out[s] = (acc * inv).astype(f16)
    return out


BIAS_ACT_FAULTS = ("sigmoid of the fp16 sum", "bias at channel % 8")


def bias_act_model(x16, bias, act, fault=None):
    assert fault is None or fault in BIAS_ACT_FAULTS
    with np.errstate(over="ignore", invalid="ignore"):
        a = x16.astype(f32)
        if bias is not None:
            bb = np.asarray(bias, f32)
            if fault == "bias at channel % 8":
                bb = bb[np.arange(bb.size) % 8]
            a = a + bb
        if act == 1:
            a = relu_keep_nan(a)
        if act == 2:
            a = _sigmoid32(a.astype(f16).astype(f32) if fault == "sigmoid of the fp16 sum" else a)
        return a.astype(f16)
