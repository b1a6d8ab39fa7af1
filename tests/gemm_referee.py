"""A float64 referee for the tracker's matrix-core convolutions and GEMMs (CPU only: numpy + torch float64).

Every kernel of the family multiplies fp16 operands exactly, accumulates in fp32 in some order and rounds once to fp16.
For the very operands a kernel reads this module gives
  ref  the operation in float64,
  mag  the same operation on absolute values (|bias| included),
  K    the number of terms of one output,
and a BASELINE: the operation in float32 on the CPU (F.conv2d / matmul / einsum), rounded once to fp16.  `gate` then
asserts a rigorous worst-case bound and two statistical ones that are measured against the baseline: a kernel may sum in
another order than the CPU does, but it may not round where the baseline does not.

    hard    |y - ref| <= 1/2 ulp16(ref) (1 + 2^-10) + K 2^-23 mag       (any order of fp32 additions, doubled because the
                                                                         matrix core's adder is not documented as RN)
    flips   share of y != round16(ref)  <=  2 x the baseline's + 2e-3    (a flip needs the fp32 error to straddle an fp16
                                                                         rounding boundary; a systematic fault gives ~1/2)
    excess  x = max(0, |y - ref| - 1/2 ulp16(ref)) / mag: max(x) and quantile(x, 0.999) <= 8 x the baseline's + 2^-24

Only elements whose round16(ref) is finite are looked at.  Where a kernel documents an fp16 rounding point before the end,
the reference and the baseline apply it (`two_step`) and the same three bounds hold unchanged.  There a correct kernel
can round the intermediate value to the other neighbour than the reference does (its fp32 sum lies across an fp16
boundary from the float64 one) and is then off by a whole ulp of the intermediate, ~1e-4 of mag: the baseline does the
same on a few elements in 10^4, so its own max excess is that large and the MAX-excess gate is blunt for such an
operation; the flip share and the p99.9 excess stay sharp (with bias + ReLU a truncating last conversion gives 0.24 --
half of the outputs the ReLU leaves -- and 1.5e-5 .. 4.4e-5, tests/test_gemm_referee_cpu.py).  At C = 128 the hard bound's
K 2^-23 mag term happens to cover that whole ulp; for the shorter sums of the frame encoders (K = 32 .. 288 with an fp16
bias) it does not, and `two_step_slack` adds it for exactly the elements that can round either way (`slack`)."""
import numpy as np
import torch
import torch.nn.functional as F

FLIP_FACTOR, FLIP_FLOOR = 2.0, 2e-3
EXCESS_FACTOR, EXCESS_FLOOR = 8.0, 2.0 ** -24


def round16(a):
    """float64 -> the nearest fp16 (one rounding; overflow gives +-inf), returned as float64"""
    with np.errstate(over="ignore"):
        return np.asarray(a, dtype=np.float64).astype(np.float16).astype(np.float64)


def ulp16(r):
    """spacing of fp16 at |r|: 2^(floor(log2(max(|r|, 2^-14))) - 10)"""
    a = np.maximum(np.abs(np.asarray(r, dtype=np.float64)), 2.0 ** -14)
    return np.exp2(np.floor(np.log2(a)) - 10.0)


def hard_bound(ref, mag, K, slack=None):
    b = 0.5 * ulp16(ref) * (1.0 + 2.0 ** -10) + K * 2.0 ** -23 * mag
    return b if slack is None else b + slack


def two_step_slack(pre_ref, pre_mag, K, ref):
    """The allowance of a two-step operation whose K is too small for the hard bound's K 2^-23 mag term to cover an
    intermediate rounding that lands on the other neighbour (see `two_step`; at K = 32 .. 288 even the fp32 baseline
    misses the unwidened bound, by up to 1.7 x).  Only an element whose float64 intermediate lies within the fp32
    summation error (2 K 2^-23 mag, the hard bound's own term) of an fp16 rounding boundary can round the other way; it
    is then off by one spacing of the intermediate, and the last rounding acts on that other value: slack =
    ulp16(pre) + 1/2 ulp16(ref) there and 0 on every other element, for which the bound stays as it is.  That is 5 % of
    the elements at K = 32 but nearly all from K ~ 200 on (the worst-case fp32 error is then as large as the spacing):
    there the hard bound is ~1.5 ulp and blunt, the flip share and the p99.9 excess stay sharp, and the GPU test pins
    the second rounding exactly (the CPU's fp16 add applied to the kernel's own bias-free output)."""
    dist = 0.5 * ulp16(pre_ref) - np.abs(pre_ref - round16(pre_ref))
    near = dist <= 2.0 * K * 2.0 ** -23 * pre_mag
    return np.where(near, ulp16(pre_ref) + 0.5 * ulp16(ref), 0.0)


def measure(y16, ref, mag, K, where=None, slack=None):
    """(flip share, max excess, p99.9 excess, largest |y - ref| / hard bound) over the elements with finite round16(ref)
    (and, with `where`, inside that mask)"""
    y = np.asarray(y16).astype(np.float64).reshape(-1)
    ref = np.asarray(ref, dtype=np.float64).reshape(-1)
    mag = np.asarray(mag, dtype=np.float64).reshape(-1)
    r16 = round16(ref)
    sel = np.isfinite(r16)
    if where is not None:
        sel = sel & np.asarray(where, dtype=bool).reshape(-1)
    assert sel.any(), "no finite reference element"
    y, ref, mag, r16 = y[sel], ref[sel], mag[sel], r16[sel]
    slack = None if slack is None else np.asarray(slack, dtype=np.float64).reshape(-1)[sel]
    with np.errstate(invalid="ignore"):
        err = np.abs(y - ref)
    err = np.where(np.isfinite(y), err, np.inf)
    bound = hard_bound(ref, mag, K, slack)
    over = np.maximum(0.0, err - 0.5 * ulp16(ref))
    with np.errstate(divide="ignore", invalid="ignore"):
        x = np.where(over > 0.0, over / mag, 0.0)
    return {"flip": float(np.mean(y != r16)), "max": float(x.max()), "p999": float(np.quantile(x, 0.999)),
            "hard": float((err / bound).max()), "worst": int(np.flatnonzero(sel)[int(np.argmax(err / bound))])}


def gate(y16, ref, mag, K, baseline16, label="", where=None, slack=None):
    """asserts the three bounds of the module's docstring; returns the six measured numbers (kernel and baseline: flip
    share, max excess, p99.9 excess) and both largest ratios to the hard bound"""
    k = measure(y16, ref, mag, K, where, slack)
    b = measure(baseline16, ref, mag, K, where, slack)
    res = {"flip": k["flip"], "flip_base": b["flip"], "max": k["max"], "max_base": b["max"], "p999": k["p999"],
           "p999_base": b["p999"], "hard": k["hard"], "hard_base": b["hard"], "worst": k["worst"]}
    res["line"] = (f"{label}: flips {k['flip']:.3e} (base {b['flip']:.3e})  max excess {k['max']:.2e} ({b['max']:.2e})  "
                   f"p99.9 {k['p999']:.2e} ({b['p999']:.2e})  hard {k['hard']:.3f} ({b['hard']:.3f})")
    assert b["hard"] <= 1.0, f"{label}: the fp32 baseline misses the hard bound ({b['hard']:.3g}): the referee is wrong"
    missed = _missed(k, b)
    assert not missed, f"{res['line']}\n  misses {sorted(missed)}; largest hard-bound ratio at flat element {k['worst']}"
    return res


def failed_assertions(y16, ref, mag, K, baseline16, slack=None):
    """which of the gate's assertions a result misses: a subset of {"hard", "flip", "excess"}"""
    return _missed(measure(y16, ref, mag, K, slack=slack), measure(baseline16, ref, mag, K, slack=slack))


def _missed(k, b):
    out = set()
    if k["hard"] > 1.0:
        out.add("hard")
    if k["flip"] > FLIP_FACTOR * b["flip"] + FLIP_FLOOR:
        out.add("flip")
    if k["max"] > EXCESS_FACTOR * b["max"] + EXCESS_FLOOR or k["p999"] > EXCESS_FACTOR * b["p999"] + EXCESS_FLOOR:
        out.add("excess")
    return out


# ---------------------------------------------------------------------------------------------- operand regimes

def operands(regime, x_shape, w_shape, w_div, seed):
    """(x, w) fp16 torch tensors; x_shape = [..., C] (channels last), w_shape = [O, ...], w_div = 3 sqrt(C) or sqrt(K).
      plain      x = randn, w = randn / w_div
      offset     x = 8 + randn / 8, w as above minus its per-output-channel mean: results cancel to ~5e-4 of mag
      subnormal  x = k 2^-20, k = 1 .. 15 (exact fp16 subnormals), w = 64 randn: every product is exact in fp32"""
    g = torch.Generator().manual_seed(seed)
    if regime == "plain":
        x = torch.randn(x_shape, generator=g)
        w = torch.randn(w_shape, generator=g) / w_div
    elif regime == "offset":
        x = 8.0 + torch.randn(x_shape, generator=g) / 8.0
        w = torch.randn(w_shape, generator=g) / w_div
        w = w - w.reshape(w_shape[0], -1).mean(1).reshape([-1] + [1] * (len(w_shape) - 1))
    elif regime == "subnormal":
        x = torch.randint(1, 16, x_shape, generator=g).double() * 2.0 ** -20
        w = 64.0 * torch.randn(w_shape, generator=g)
    else:
        raise ValueError(regime)
    return x.half(), w.half()


# ---------------------------------------------------------------------------------------------- references

def _conv(x, w):
    """3x3 / pad 1: x [n,h,w,C], w [O,C,3,3] (one dtype) -> [n,h,w,O]"""
    return F.conv2d(x.permute(0, 3, 1, 2), w, padding=1).permute(0, 2, 3, 1).contiguous()


def conv3x3_ref(x16, w16):
    """(ref, mag, K, baseline16) of the bias-free 3x3 convolution of NHWC fp16 x with fp16 w [O,C,3,3].  K counts the
    terms of an interior pixel; border pixels have fewer non-zero ones."""
    with np.errstate(all="ignore"):
        ref = _conv(x16.double(), w16.double()).numpy()
        mag = _conv(x16.double().abs(), w16.double().abs()).numpy()
        base = _conv(x16.float(), w16.float()).half().numpy()
    return ref, mag, 9 * x16.shape[-1], base


def conv_ref(x16, w16, ksize, stride, bias=None, relu=False, with_slack=False):
    """(ref, mag, K, baseline16[, slack]) of act(conv(x) + b) as [n,ho,wo,O]: NHWC fp16 x [n,h,w,C], fp16 w [O,C,k,k], padding
    ksize // 2, stride 1 or 2; K = ksize^2 C counts the terms of an interior pixel.  The bias joins where the kernels
    document it, told by its dtype:
      fp16 bias (gs_enc_conv): added AFTER the fp16 rounding of the convolution, half(half(conv) + b) -- `two_step`;
      fp32 bias (gs_conv7x7_c4): in the fp32 accumulator before the ONE rounding, K + 1 terms.
    ReLU commutes with the last rounding and is applied to the reference and the baseline alike.  with_slack: also the
    gate's `slack` (two_step_slack for the fp16 bias, None otherwise)."""
    assert w16.shape[2] == w16.shape[3] == ksize and x16.dtype == torch.float16 and w16.dtype == torch.float16

    def cv(x, w):
        return F.conv2d(x.permute(0, 3, 1, 2), w, stride=stride, padding=ksize // 2).permute(0, 2, 3, 1).contiguous()

    with np.errstate(all="ignore"):
        ref = cv(x16.double(), w16.double()).numpy()
        mag = cv(x16.double().abs(), w16.double().abs()).numpy()
        base32 = cv(x16.float(), w16.float())
    K = ksize * ksize * x16.shape[-1]
    act = (lambda p: np.maximum(p, 0.0)) if relu else (lambda p: p)
    extra = (None,) if with_slack else ()
    if bias is None:
        return (act(ref), mag, K, torch.relu(base32).half().numpy() if relu else base32.half().numpy()) + extra
    b64 = bias.double().numpy()
    if bias.dtype == torch.float16:
        pre, pmag = ref, mag
        ref, base = two_step(pre, base32.half().numpy(), lambda p: act(p + b64))
        extra = (two_step_slack(pre, pmag, K, ref),) if with_slack else ()
        return (ref, pmag + np.abs(b64), K + 1, base) + extra
    assert bias.dtype == torch.float32
    base32 = base32 + bias
    return (act(ref + b64), mag + np.abs(b64), K + 1, (torch.relu(base32) if relu else base32).half().numpy()) + extra


def two_step(pre_ref, pre_base, fn):
    """An operation with a documented fp16 rounding of the GEMM result `pre` before `fn` (elementwise, float64 ->
    float64, exact on its operands: fp16 + fp32 fits float64) and the final rounding.  ref = fn(round16(pre_ref)); the
    baseline is fn of the fp16 baseline of `pre`, rounded to fp32 (the kernel's one fp32 operation) and then to fp16.
    The gate's hard bound is not widened: a correct kernel whose intermediate rounding lands on the other neighbour is off
    by ulp16(pre), and the bound's K 2^-23 mag term is that large at the shapes the tests use (C = 128: 2.9e-3 against
    ulp16 = 2e-3 for |pre| < 4, which 4 sigma of the operands stay below).  Returns (ref, baseline16)."""
    with np.errstate(over="ignore"):
        base = fn(np.asarray(pre_base).astype(np.float64)).astype(np.float32).astype(np.float16)
    return fn(round16(pre_ref)), base


def gemm_ref(x16, w16, bias=None, relu=False):
    """(ref, mag, K, baseline16) of y[p, o] = act(sum_k x[p, k] w[o, k] + b[o]); x [rows, k], w [O, k] fp16, b fp32"""
    xd, wd = x16.double(), w16.double()
    ref = (xd @ wd.t()).numpy()
    mag = (xd.abs() @ wd.abs().t()).numpy()
    base = x16.float() @ w16.float().t()
    K = x16.shape[1]
    if bias is not None:
        ref = ref + bias.double().numpy()
        mag = mag + bias.double().abs().numpy()
        base = base + bias.float()
        K += 1
    if relu:
        ref = np.maximum(ref, 0.0)
        base = torch.relu(base)
    return ref, mag, K, base.half().numpy()


def corr_ref(f1, f2):
    """level 0 of the correlation volume: f1, f2 fp16 [n,128,h,w]; both maps are divided by 4 IN FP16 (corr_prep_kernel),
    then ref[e,p1,p2] = sum_c f1[e,c,p1] f2[e,c,p2] -> (ref, mag, K, baseline16) as [n,h,w,h,w]"""
    n, c, h, w = f1.shape
    q1 = torch.from_numpy(f1.numpy().astype(np.float16) / np.float16(4)).reshape(n, c, h * w)
    q2 = torch.from_numpy(f2.numpy().astype(np.float16) / np.float16(4)).reshape(n, c, h * w)
    assert q1.dtype == torch.float16
    ref = torch.einsum("ncp,ncq->npq", q1.double(), q2.double()).numpy()
    mag = torch.einsum("ncp,ncq->npq", q1.double().abs(), q2.double().abs()).numpy()
    base = torch.einsum("ncp,ncq->npq", q1.float(), q2.float()).half().numpy()
    s = (n, h, w, h, w)
    return ref.reshape(s), mag.reshape(s), c, base.reshape(s)


def altcorr_ref(pyr, coords, ii, jj):
    """gs_altcorr_pyramid: pyr = 4 fp16 tensors [N, H >> l, W >> l, 128] (the rows the kernel reads), coords fp32
    [E,H,W,2], ii / jj int64 [E].  Per level the dot products of source pixel p with the 8 x 8 window at
    floor(coords / 2^l) - 3 (0 outside the map) in float64, blended with the four bilinear weights computed in FP32 from the
    fp32 coordinates; channel 49 l + 7 ix + iy.  Coordinates must be finite.  -> (ref, mag, K = 132, baseline16) as
    [E,H,W,196]; the baseline is the same formula in fp32."""
    E, H, W, _ = coords.shape
    f1 = pyr[0][ii].reshape(E, H * W, 128)
    c = coords.numpy().astype(np.float32).reshape(E, H * W, 2)
    ref = np.zeros((E, H * W, 196))
    mag = np.zeros((E, H * W, 196))
    base = np.zeros((E, H * W, 196), dtype=np.float32)
    ar = torch.arange(8)
    for l in range(4):
        f2 = pyr[l][jj]
        H2, W2 = f2.shape[1:3]
        inv = np.float32(1.0 / (1 << l))
        cx, cy = c[..., 0] * inv, c[..., 1] * inv
        fx, fy = np.floor(cx), np.floor(cy)
        dx, dy = (cx - fx).astype(np.float32), (cy - fy).astype(np.float32)
        x = torch.from_numpy(fx.astype(np.int64) - 3)[..., None, None] + ar[None, None, None, :]       # [E,P,1,8]
        y = torch.from_numpy(fy.astype(np.int64) - 3)[..., None, None] + ar[None, None, :, None]       # [E,P,8,1]
        inside = ((x >= 0) & (x < W2) & (y >= 0) & (y < H2)).expand(E, H * W, 8, 8)
        idx = (y.clamp(0, H2 - 1) * W2 + x.clamp(0, W2 - 1)).expand(E, H * W, 8, 8).reshape(E, -1)     # [E, P*64]
        win = torch.gather(f2.reshape(E, H2 * W2, 128), 1, idx[..., None].expand(E, idx.shape[1], 128))
        win = win.reshape(E, H * W, 64, 128) * inside.reshape(E, H * W, 64, 1).to(win.dtype)
        one = np.float32(1.0)
        wts = [(one - dy) * (one - dx), (one - dy) * dx, dy * (one - dx), dy * dx]                     # fp32, as the kernel
        assert all(t.dtype == np.float32 for t in wts)
        for kind in ("ref", "mag", "base"):
            if kind == "base":
                d = torch.einsum("epc,epkc->epk", f1.float(), win.float()).numpy()
            elif kind == "ref":
                d = torch.einsum("epc,epkc->epk", f1.double(), win.double()).numpy()
            else:
                d = torch.einsum("epc,epkc->epk", f1.double().abs(), win.double().abs()).numpy()
            d = d.reshape(E, H * W, 8, 8)                                                              # [iy][ix]
            taps = [d[:, :, :7, :7], d[:, :, :7, 1:], d[:, :, 1:, :7], d[:, :, 1:, 1:]]
            if kind == "base":
                o = sum(t * wt[..., None, None] for t, wt in zip(taps, wts))
                assert o.dtype == np.float32
            else:
                o = sum(t * wt.astype(np.float64)[..., None, None] for t, wt in zip(taps, wts))
            o = o.transpose(0, 1, 3, 2).reshape(E, H * W, 49)                                          # 7 ix + iy
            {"ref": ref, "mag": mag, "base": base}[kind][..., 49 * l:49 * l + 49] = o
    s = (E, H, W, 196)
    return ref.reshape(s), mag.reshape(s), 132, base.astype(np.float16).reshape(s)


# ---------------------------------------------------------------------------------------------- CPU models of a kernel

def conv3x3_kernel_order(x16, w16, round_chunks=False):
    """fp32 accumulation in gs_conv3x3_pp's order: 32-channel chunks outer, the 9 taps inner, one fp32 addition per step
    (a step = the fp32 dot product over the chunk's 32 channels) -> fp32 [n,h,w,O].  round_chunks: the accumulator is
    rounded to fp16 after every chunk (a wrong kernel)."""
    n, h, w, c = x16.shape
    xp = F.pad(x16.float(), (0, 0, 1, 1, 1, 1))
    wf = w16.float()
    acc = torch.zeros(n, h, w, w16.shape[0])
    for ck in range(c // 32):
        for ky in range(3):
            for kx in range(3):
                acc = acc + xp[:, ky:ky + h, kx:kx + w, 32 * ck:32 * ck + 32] @ wf[:, 32 * ck:32 * ck + 32, ky, kx].t()
        if round_chunks:
            acc = acc.half().float()
    return acc


def truncate16(a32):
    """fp32 -> fp16 rounding toward zero (a wrong conversion)"""
    a = a32.numpy().astype(np.float32)
    with np.errstate(over="ignore"):
        r = a.astype(np.float16)
    away = np.abs(r.astype(np.float32)) > np.abs(a)
    return np.where(away, np.nextafter(r, np.float16(0)), r).astype(np.float16)
