"""The implicit-GEMM kernels of the update operator and of the correlation path against float64, per element.

gs_conv3x3_pp and its bias + ReLU / merged-head epilogues, gs_conv1x1, gs_corr_lookup_enc, level 0 of
gs_corr_volume_pyramid, gs_altcorr_pyramid, gs_enc_conv (all ten layer shapes of the frame encoders) and gs_conv7x7_c4
(the flow encoder's stem) each run on seeded fp16 operands; tests/gemm_referee.py computes, on the CPU
and from the same fp16 operands, the float64 result, its magnitude sum and an fp32 baseline, and its `gate` asserts the
worst-case fp32 bound plus the two statistical bounds (rounding flips, excess over half an ulp) that separate "another
summation order" from "a rounding the kernel's header does not document" -- tests/test_gemm_referee_cpu.py shows that an
fp16 accumulator hand-over, a truncating conversion, an unpadded image seam, a stem that drops a border-straddling tap
pair and a stride-2 kernel on the odd pixels fail them.  Nothing computed on the GPU acts as referee.  Every gate prints
its figures (kernel and baseline side by side).  The window lookups whose features gs_corr_lookup_enc multiplies have
their own judge, tests/test_lookup_numerics_gpu.py.

MEASURED for gs_enc_conv and gs_conv7x7_c4 (MI355X; kernel (baseline), the largest over the runs of a row):
  (k, c_in, c_out, stride)     bias      gates  flip share          max excess          p99.9 excess        hard-bound ratio
  enc_conv (7, 4, 32, 2)       no bias     6    6.2e-04 (1.6e-03)   1.6e-08 (3.9e-08)   0.0e+00 (2.5e-09)   0.861 (0.861)
  enc_conv (7, 4, 32, 2)       fp16 bias   6    5.4e-04 (8.9e-04)   6.0e-05 (8.4e-05)   0.0e+00 (0.0e+00)   0.942 (0.942)
  enc_conv (3, 32, 32, 1)      no bias     4    1.6e-02 (3.3e-02)   2.2e-08 (6.1e-08)   8.4e-09 (3.0e-08)   0.784 (0.784)
  enc_conv (3, 32, 32, 1)      fp16 bias   4    3.0e-03 (7.0e-03)   4.6e-05 (6.8e-05)   4.9e-07 (5.8e-07)   0.792 (0.792)
  enc_conv (3, 32, 64, 2)      no bias     4    1.2e-02 (2.7e-02)   1.4e-08 (8.1e-08)   7.1e-09 (2.5e-08)   0.788 (0.788)
  enc_conv (3, 32, 64, 2)      fp16 bias   4    2.4e-03 (5.7e-03)   7.2e-05 (8.9e-05)   1.4e-07 (6.2e-07)   0.845 (0.845)
  enc_conv (3, 64, 64, 1)      no bias     4    2.2e-02 (4.7e-02)   2.6e-08 (8.5e-08)   1.0e-08 (3.4e-08)   0.599 (0.599)
  enc_conv (3, 64, 64, 1)      fp16 bias   4    4.3e-03 (9.7e-03)   5.5e-05 (9.3e-05)   4.0e-07 (6.8e-07)   0.444 (0.487)
  enc_conv (3, 64, 128, 2)     no bias     4    1.6e-02 (3.7e-02)   2.1e-08 (7.9e-08)   8.0e-09 (2.9e-08)   0.607 (0.607)
  enc_conv (3, 64, 128, 2)     fp16 bias   4    2.9e-03 (8.9e-03)   3.0e-05 (3.0e-05)   2.0e-07 (5.9e-07)   0.309 (0.336)
  enc_conv (3, 128, 128, 1)    no bias     6    2.8e-02 (6.0e-02)   2.9e-08 (1.2e-07)   1.0e-08 (3.2e-08)   0.349 (0.349)
  enc_conv (3, 128, 128, 1)    fp16 bias   6    5.6e-03 (1.5e-02)   5.6e-05 (5.6e-05)   2.8e-07 (5.0e-07)   0.400 (0.400)
  enc_conv (1, 32, 64, 2)      no bias     4    1.0e-02 (1.7e-02)   2.1e-08 (3.4e-08)   8.8e-09 (1.7e-08)   0.981 (0.981)
  enc_conv (1, 32, 64, 2)      fp16 bias   4    1.4e-03 (2.7e-03)   2.2e-04 (2.2e-04)   2.4e-07 (3.7e-07)   0.987 (0.987)
  enc_conv (1, 64, 128, 2)     no bias     4    1.4e-02 (2.4e-02)   2.0e-08 (5.0e-08)   8.2e-09 (2.4e-08)   0.962 (0.962)
  enc_conv (1, 64, 128, 2)     fp16 bias   4    2.6e-03 (4.2e-03)   8.6e-05 (9.7e-05)   4.7e-07 (9.7e-07)   0.967 (0.967)
  enc_conv (1, 128, 128, 1)    no bias     4    1.6e-02 (3.1e-02)   3.1e-08 (9.7e-08)   9.1e-09 (2.6e-08)   0.912 (0.912)
  enc_conv (1, 128, 128, 1)    fp16 bias   4    2.9e-03 (5.6e-03)   1.2e-04 (2.3e-04)   3.9e-07 (8.1e-07)   0.939 (0.939)
  enc_conv (1, 128, 256, 1)    no bias     4    1.6e-02 (3.1e-02)   3.2e-08 (8.3e-08)   9.1e-09 (2.8e-08)   0.913 (0.913)
  enc_conv (1, 128, 256, 1)    fp16 bias   4    2.5e-03 (5.9e-03)   2.3e-04 (2.6e-04)   4.0e-07 (8.0e-07)   0.935 (0.935)
  conv7x7_c4                   fp32 bias  12    6.3e-03 (1.1e-02)   2.1e-07 (1.2e-07)   6.2e-09 (1.8e-08)   0.948 (0.948)
  With the fp16 bias the max excess is an intermediate rounding on the other neighbour (the baseline's is as large) and
  the hard bound carries gemm_referee.two_step_slack; the second rounding itself is asserted exactly.  None of these
  figures is a tolerance: the bounds are the gate's own factors over the CPU baseline."""
import numpy as np
import pytest
import torch

import gemm_referee as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = 7.0


@pytest.fixture(autouse=True)
def _stop_after_a_device_error():
    """a failed assertion lets the next test run; a device error ends the session (nothing more is launched after it)"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as exc:
        pytest.exit(f"device error, stopping: {exc}", returncode=3)


def _report(res):
    print(res["line"])
    return res


# ------------------------------------------------------------------------------------------------ gs_conv3x3_pp

# (n, h, w, C, x_stride, n_out, tw)
PP_CASES = [(2, 5, 19, 32, 32, 128, 16),      # one chunk (no prefetch ring), tiles span images, partial tile in x
            (3, 7, 9, 64, 72, 256, 8),        # channel slice of wider rows, two output blocks, TW = 8
            (2, 33, 16, 128, 128, 64, 16),    # BN = 64; taller than a tile's 32 rows: a tile seam inside an image
            (3, 7, 19, 320, 320, 256, 16),    # ten chunks: the production K
            (2, 9, 20, 128, 128, 384, 16)]    # three output blocks
PP_RUNS = [(c, r) for c in PP_CASES for r in ("plain", "offset")] + [(PP_CASES[0], "subnormal"), (PP_CASES[3], "subnormal")]


def _strided(x16, stride, fill=3.0):
    """[..., C] fp16 -> the same values as the first C channels of rows `stride` halves apart (device tensor)"""
    c = x16.shape[-1]
    buf = torch.full(tuple(x16.shape[:-1]) + (stride,), fill, dtype=torch.float16)
    buf[..., :c] = x16
    return buf.to(DEV)


def _run_pp(xbuf, c, wt16, n_out, tw, xcd):
    """gs_conv3x3_pp on the first c channels of xbuf [n,h,w,x_stride]; y rows are n_out + 8 apart, the 8 sentinel columns
    are checked"""
    from go_slam_amd import _lib
    from go_slam_amd.droid_net import pack_conv3x3_weight
    n, h, w, xs = xbuf.shape
    wp = pack_conv3x3_weight(wt16.to(DEV), 32)
    y = torch.full((n, h, w, n_out + 8), SENTINEL, dtype=torch.float16, device=DEV)
    rc = _lib.lib().gs_conv3x3_pp(_lib.ptr(xbuf), xs, c, _lib.ptr(wp), tw, _lib.ptr(y), n_out + 8, n_out, n, h, w, xcd,
                                  _lib.stream_ptr(DEV))
    _lib.check(rc, "conv3x3_pp")
    torch.cuda.synchronize()
    y = y.cpu()
    assert bool((y[..., n_out:] == SENTINEL).all()), "the kernel wrote outside its channels"
    return y[..., :n_out].contiguous()


@pytest.mark.parametrize("case,regime", PP_RUNS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v)
def test_conv3x3_pp_per_element(built_lib, case, regime):
    """both workgroup orders; in the subnormal regime a kernel that flushes fp16 subnormal operands returns zeros"""
    n, h, w, c, xs, n_out, tw = case
    x, wt = R.operands(regime, (n, h, w, c), (n_out, c, 3, 3), 3.0 * c ** 0.5, seed=1000 * n + c + w)
    ref, mag, K, base = R.conv3x3_ref(x, wt)
    if regime == "subnormal":
        assert float(x.float().max()) < 2.0 ** -14 and float(np.median(np.abs(ref))) > 2.0 ** -10
    xbuf = _strided(x, xs)
    for xcd in (0, 1):
        y = _run_pp(xbuf, c, wt, n_out, tw, xcd)
        _report(R.gate(y.numpy(), ref, mag, K, base, label=f"conv3x3_pp {case} {regime} xcd={xcd}"))


def _big_weights(shape, div, g):
    """randn / div with every magnitude at least 2^-10 (no product with a non-finite input is 0 x inf by a zero weight)"""
    w = torch.randn(shape, generator=g) / div
    return torch.where(w < 0, -w.abs().clamp_min(2.0 ** -10), w.abs().clamp_min(2.0 ** -10)).half()


def test_conv3x3_pp_non_finite_inputs_stay_in_their_own_image(built_lib):
    """+inf at the last pixel of image 0 and NaN at the first pixel of image 1 -- neighbours in the row-stacked tiling:
    non-finite outputs are exactly the two 3 x 3 neighbourhoods clipped to their own image, in every channel; every other
    output is bit-equal to the run without the poison."""
    n, h, w, c, xs, n_out, tw = PP_CASES[0]
    g = torch.Generator().manual_seed(77)
    x = torch.randn(n, h, w, c, generator=g).half()
    wt = _big_weights((n_out, c, 3, 3), 3.0 * c ** 0.5, g)
    assert float(wt.abs().min()) >= 2.0 ** -10
    xp = x.clone()
    xp[0, h - 1, w - 1, 3] = float("inf")
    xp[1, 0, 0, 17] = float("nan")
    want = torch.zeros(n, h, w, dtype=torch.bool)
    want[0, h - 2:, w - 2:] = True
    want[1, :2, :2] = True
    for xcd in (0, 1):
        clean = _run_pp(x.to(DEV), c, wt, n_out, tw, xcd)
        got = _run_pp(xp.to(DEV), c, wt, n_out, tw, xcd)
        assert bool(torch.isfinite(clean).all())
        bad = ~torch.isfinite(got)
        assert torch.equal(bad, want[..., None].expand_as(bad)), \
            f"xcd={xcd}: non-finite pixels {bad.any(-1).nonzero().tolist()}, partly in {int((bad.any(-1) != bad.all(-1)).sum())}"
        assert bool(torch.isnan(got[1, :2, :2]).all())
        assert torch.equal(got[~bad].view(torch.int16), clean[~bad].view(torch.int16)), f"xcd={xcd}"


def test_conv3x3_pp_overflow_stores_infinity(built_lib):
    """where round16(ref) is +-inf the kernel stores that infinity (not NaN, not 65504); everything finite passes the gate.
    Elements whose |ref| lies within the hard bound of 65520 (the fp16 overflow threshold) may go either way and are left
    out: fewer than 1e-3 of all."""
    n, h, w, c, xs, n_out, tw = PP_CASES[0]
    g = torch.Generator().manual_seed(78)
    x = (8192.0 * torch.randn(n, h, w, c, generator=g)).half()
    wt = (4.0 * _big_weights((n_out, c, 3, 3), 3.0 * c ** 0.5, g).float()).half()
    assert bool(torch.isfinite(x).all())
    ref, mag, K, base = R.conv3x3_ref(x, wt)
    r16 = R.round16(ref)
    near = np.abs(np.abs(ref) - 65520.0) <= R.hard_bound(ref, mag, K)
    over = np.isinf(r16) & ~near
    print(f"overflow: {int(over.sum())} of {ref.size} elements overflow, {int(near.sum())} left out")
    assert over.mean() > 0.01 and (r16[over] > 0).any() and (r16[over] < 0).any() and near.mean() < 1e-3
    for xcd in (0, 1):
        y = _run_pp(x.to(DEV), c, wt, n_out, tw, xcd).numpy()
        assert np.array_equal(y[over].astype(np.float64), r16[over]), \
            f"xcd={xcd}: {int((y[over].astype(np.float64) != r16[over]).sum())} overflowing elements are not +-inf"
        _report(R.gate(y, ref, mag, K, base, where=~near, label=f"conv3x3_pp overflow xcd={xcd}"))


# ------------------------------------------------------------------------------------- gs_conv3x3_bias_relu / heads

@pytest.mark.parametrize("n_out,y_stride,y_off", [(128, 320, 128), (64, 72, 0)])
@pytest.mark.parametrize("regime", ["plain", "offset"])
def test_conv3x3_bias_relu_per_element(built_lib, n_out, y_stride, y_off, regime):
    """csrc/conv3x3_pp.hip, EPI 3: the fp32 accumulators are rounded to fp16, then y = fp16(relu(float(pre) + bias)) -- the
    rounding points of gs_conv3x3_pp followed by gs_bias_act.  The reference rounds where the kernel does: ref =
    relu(round16(conv) + b), and so does the baseline (gemm_referee.two_step); the gate's bounds are unchanged, with K =
    9 C + 1 for the fp32 addition of the bias.  Of the excess gates only p99.9 is sharp here (see gemm_referee).  128 -> 128
    into channels 128:256 of a 320-wide destination, 128 -> 64 (BN = 64) with 8 sentinel columns; the rest stays untouched."""
    from go_slam_amd import _lib
    from go_slam_amd.droid_net import pack_conv3x3_weight
    n, h, w, c = 2, 9, 20, 128
    x, wt = R.operands(regime, (n, h, w, c), (n_out, c, 3, 3), 3.0 * c ** 0.5, seed=310 + n_out)
    bias = 0.3 * torch.randn(n_out, generator=torch.Generator().manual_seed(311))
    pre, pmag, K, pbase = R.conv3x3_ref(x, wt)
    b64 = bias.double().numpy()
    ref, base = R.two_step(pre, pbase, lambda p: np.maximum(p + b64, 0.0))
    mag = pmag + np.abs(b64)
    xd, wp, bd = x.to(DEV), pack_conv3x3_weight(wt.to(DEV), 32), bias.to(DEV)
    y = torch.full((n, h, w, y_stride), SENTINEL, dtype=torch.float16, device=DEV)
    rc = _lib.lib().gs_conv3x3_bias_relu(_lib.ptr(xd), c, c, _lib.ptr(wp), _lib.ptr(bd), y.data_ptr() + 2 * y_off, y_stride,
                                         n_out, n, h, w, _lib.stream_ptr(DEV))
    _lib.check(rc, "conv3x3_bias_relu")
    torch.cuda.synchronize()
    y = y.cpu()
    assert bool((y[..., :y_off] == SENTINEL).all()) and bool((y[..., y_off + n_out:] == SENTINEL).all())
    got = y[..., y_off:y_off + n_out].contiguous().numpy()
    assert 0.2 < float((got == 0).mean()) < 0.8
    _report(R.gate(got, ref, mag, K + 1, base, label=f"conv3x3_bias_relu 128->{n_out} {regime}"))


@pytest.mark.parametrize("tw", [8, 16])
@pytest.mark.parametrize("regime", ["plain", "offset"])
def test_conv3x3_heads_stored_block_per_element(built_lib, tw, regime):
    """gs_conv3x3_heads, 128 -> 384 with n_tap_blocks = 2: the third 128-channel block is stored to y as gs_conv3x3_pp
    stores it (the tap products of the first two keep their equality test in test_conv3x3_mfma_shape_gpu.py)."""
    from go_slam_amd import _lib
    import go_slam_amd.droid_net as DN
    n, h, w, c, n_out = 2, 9, 20, 128, 384
    x, wt = R.operands(regime, (n, h, w, c), (n_out, c, 3, 3), 3.0 * c ** 0.5, seed=410 + tw)
    g = torch.Generator().manual_seed(411)
    tapw = DN.pack_heads_tap_weights([(torch.randn(2, 128, 3, 3, generator=g) / 12.0).to(DEV) for _ in range(2)])
    in_bias = (0.3 * torch.randn(256, generator=g)).to(DEV)
    ref, mag, K, base = R.conv3x3_ref(x, wt[256:])
    xd, wp = x.to(DEV), DN.pack_conv3x3_weight(wt.to(DEV), 32)
    ts, rs = DN.heads_workspace_shapes(n, h, w, n_out, 2)
    taps = torch.full(ts, float("nan"), dtype=torch.float32, device=DEV)
    y = torch.full((n, h, w, 128 + 8), SENTINEL, dtype=torch.float16, device=DEV)
    rc = _lib.lib().gs_conv3x3_heads(_lib.ptr(xd), c, c, _lib.ptr(wp), tw, _lib.ptr(tapw), _lib.ptr(in_bias), 2,
                                     _lib.ptr(taps), _lib.ptr(y), 128 + 8, n_out, n, h, w, _lib.stream_ptr(DEV))
    _lib.check(rc, "conv3x3_heads")
    torch.cuda.synchronize()
    y = y.cpu()
    assert bool((y[..., 128:] == SENTINEL).all()) and bool(torch.isfinite(taps).all())
    _report(R.gate(y[..., :128].contiguous().numpy(), ref, mag, K, base, label=f"conv3x3_heads block 2 tw={tw} {regime}"))


# ------------------------------------------------------------------------------------------------ gs_conv1x1

@pytest.mark.parametrize("k_in,n_out,x_stride,act", [(196, 128, 196, 1), (196, 128, 208, 1), (128, 576, 128, 0),
                                                     (128, 128, 320, 0)])
@pytest.mark.parametrize("regime", ["plain", "offset"])
def test_conv1x1_per_element(built_lib, k_in, n_out, x_stride, act, regime):
    """173 rows = five 32-pixel blocks and a ragged one: the 8-byte last piece of a dense 196-wide chunk, strided rows,
    the sliced 576-channel output.  The bias joins the fp32 accumulator before the one rounding: K = k_in + 1."""
    from go_slam_amd import _lib
    from go_slam_amd.droid_net import pack_1x1_weight
    rows = 173
    x, wt = R.operands(regime, (rows, k_in), (n_out, k_in), k_in ** 0.5, seed=510 + k_in + n_out + x_stride)
    bias = 0.3 * torch.randn(n_out, generator=torch.Generator().manual_seed(511))
    ref, mag, K, base = R.gemm_ref(x, wt, bias, relu=bool(act))
    assert K == k_in + 1
    xbuf = _strided(x, x_stride)
    wp, bd = pack_1x1_weight(wt.reshape(n_out, k_in, 1, 1).to(DEV)), bias.to(DEV)
    y = torch.full((rows, n_out + 8), SENTINEL, dtype=torch.float16, device=DEV)
    rc = _lib.lib().gs_conv1x1(_lib.ptr(xbuf), x_stride, k_in, _lib.ptr(wp), _lib.ptr(bd), act, _lib.ptr(y), n_out + 8,
                               n_out, rows, _lib.stream_ptr(DEV))
    _lib.check(rc, "conv1x1")
    torch.cuda.synchronize()
    y = y.cpu()
    assert bool((y[:, n_out:] == SENTINEL).all())
    _report(R.gate(y[:, :n_out].contiguous().numpy(), ref, mag, K, base,
                   label=f"conv1x1 {k_in}->{n_out} stride {x_stride} act {act} {regime}"))


# ------------------------------------------------------------------------------------------------ correlation path

def _features(n, h, w, seed, scale=1.5):
    return (scale * torch.randn(n, 128, h, w, generator=torch.Generator().manual_seed(seed))).half()


@pytest.mark.parametrize("h,w,tile8", [(12, 20, False), (16, 32, True)])
def test_corr_lookup_enc_per_element(built_lib, h, w, tile8):
    """gs_corr_lookup_enc = relu(W feat + b) over the 196 looked-up features (K = 197).  The features are those of
    gs_corr_lookup_pyramid on the same volumes and coordinates (judged by tests/test_lookup_numerics_gpu.py); the product is
    refereed on the CPU.  Coordinates: identity + 6 px of noise, n = 2."""
    from go_slam_amd import droid_backends as db
    from go_slam_amd.corr import CorrBlock
    n = 2
    f1, f2 = _features(n, h, w, 610 + w).to(DEV)[None], _features(n, h, w, 611 + w).to(DEV)[None]
    block = CorrBlock(f1, f2, channels_last=True)
    assert block.layout == (db.CORR_TILE8 if tile8 else db.CORR_ROWMAJOR)
    g = torch.Generator().manual_seed(612)
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    coords = (torch.stack([xs, ys], -1)[None] + 6.0 * torch.randn(n, h, w, 2, generator=g))[None].to(DEV)
    wt = (torch.randn(128, 196, generator=g) / 14.0).half()
    bias = 0.3 * torch.randn(128, generator=g)
    wpad = torch.zeros(128, 208, dtype=torch.float16)
    wpad[:, :196] = wt
    feats = block(coords)[0].permute(0, 2, 3, 1).reshape(n * h * w, 196).cpu()
    y = block.lookup_encoded(coords, wpad.to(DEV), bias.to(DEV))
    torch.cuda.synchronize()
    y = y.permute(0, 2, 3, 1).reshape(n * h * w, 128).cpu()
    assert feats.dtype == torch.float16 and bool(torch.isfinite(feats).all())
    assert float(feats.float().std()) > 0.2 and float((feats != 0).float().mean()) > 0.3      # windows inside the map
    ref, mag, K, base = R.gemm_ref(feats, wt, bias, relu=True)
    assert K == 197
    _report(R.gate(y.numpy(), ref, mag, K, base, label=f"corr_lookup_enc {h}x{w} {'tile8' if tile8 else 'row-major'}"))


def _volume_levels(vols, h, w, tile8):
    """the four levels as [n,h,w,h >> l,w >> l] CPU tensors (tile8 levels 0-1 read back through corr_untile8)"""
    from go_slam_amd import droid_backends as db
    return [(db.corr_untile8(v, h >> l, w >> l) if tile8 and l < 2 else v).cpu() for l, v in enumerate(vols)]


@pytest.mark.parametrize("n,h,w,tile8", [(2, 12, 20, False), (2, 16, 32, True), (1, 8, 60, False)])
@pytest.mark.parametrize("regime", ["plain", "offset"])
def test_corr_volume_level0_per_element(built_lib, n, h, w, tile8, regime):
    """gs_corr_volume_pyramid level 0 (K = 128), every element against its own ulp.  corr_prep_kernel divides both maps by
    4 in fp16; the reference does the same.  offset: f1 shifted by a constant, each f2 pixel's 128 channels centred, so the
    dot products cancel.  (1, 8, 60): w % 8 == 4, the half-empty last column tile."""
    from go_slam_amd import droid_backends as db
    g = torch.Generator().manual_seed(710 + w)
    if regime == "plain":
        f1, f2 = 1.5 * torch.randn(n, 128, h, w, generator=g), 1.5 * torch.randn(n, 128, h, w, generator=g)
    else:
        f1 = 8.0 + torch.randn(n, 128, h, w, generator=g) / 8.0
        f2 = 1.5 * torch.randn(n, 128, h, w, generator=g)
        f2 = f2 - f2.mean(1, keepdim=True)
    f1, f2 = f1.half(), f2.half()
    ref, mag, K, base = R.corr_ref(f1, f2)
    if regime == "offset":
        assert float(np.median(np.abs(ref) / mag)) < 5e-3
    layout = db.CORR_TILE8 if tile8 else db.CORR_ROWMAJOR
    vols = db.corr_volume_pyramid(f1.to(DEV), f2.to(DEV), layout)
    torch.cuda.synchronize()
    y = _volume_levels(vols, h, w, tile8)[0]
    assert tuple(y.shape) == (n, h, w, h, w)
    _report(R.gate(y.numpy(), ref, mag, K, base, label=f"corr_volume level 0 {n}x{h}x{w} {regime}"))


@pytest.mark.parametrize("h,w,tile8", [(12, 20, False), (16, 32, True)])
def test_corr_volume_overflow(built_lib, h, w, tile8):
    """Source pixels A (all channels +128) and B (all -128) against target pixel T (all +128): the correlations 128 x 32 x 32
    = +-131072 exceed fp16.  Level 0 holds +inf at (A, T) and -inf at (B, T); levels 1-3 are avg_pool2d of the fp16 level
    below (the infinities travel down); the clean run differs only in T's features, so every element of every level that
    is not pooled from target pixel T is bit-equal to it."""
    import torch.nn.functional as F
    from go_slam_amd import droid_backends as db
    n = 2
    f1, f2 = _features(n, h, w, 810 + w), _features(n, h, w, 811 + w)
    (ay, ax), (by, bx), (ty, tx) = (1, 2), (h - 1, w - 3), (5, 9)
    f1[:, :, ay, ax] = 128.0
    f1[:, :, by, bx] = -128.0
    hot = f2.clone()
    hot[:, :, ty, tx] = 128.0
    layout = db.CORR_TILE8 if tile8 else db.CORR_ROWMAJOR
    clean = _volume_levels(db.corr_volume_pyramid(f1.to(DEV), f2.to(DEV), layout), h, w, tile8)
    got = _volume_levels(db.corr_volume_pyramid(f1.to(DEV), hot.to(DEV), layout), h, w, tile8)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(v).all()) for v in clean)
    ref, mag, K, base = R.corr_ref(f1, hot)
    r16 = R.round16(ref)
    assert np.isinf(r16).sum() == 2 * n and r16[0, ay, ax, ty, tx] == np.inf and r16[1, by, bx, ty, tx] == -np.inf
    g0 = got[0].numpy().astype(np.float64)
    assert np.array_equal(g0[np.isinf(r16)], r16[np.isinf(r16)]), g0[np.isinf(r16)]
    _report(R.gate(got[0].numpy(), ref, mag, K, base, label=f"corr_volume overflow level 0 {h}x{w}"))
    for l in range(4):
        same = torch.ones(got[l].shape, dtype=torch.bool)
        same[..., ty >> l, tx >> l] = False
        assert torch.equal(got[l][same].view(torch.int16), clean[l][same].view(torch.int16)), f"level {l}"
        if l:
            hl, wl = got[l - 1].shape[-2:]
            pooled = F.avg_pool2d(got[l - 1].reshape(-1, 1, hl, wl).float(), 2, 2).to(torch.float16)
            assert torch.equal(got[l].reshape(pooled.shape).view(torch.int16), pooled.view(torch.int16)), f"level {l} pool"
            assert float(got[l][0, ay, ax, ty >> l, tx >> l]) == float("inf")
            assert float(got[l][1, by, bx, ty >> l, tx >> l]) == float("-inf")


# ------------------------------------------------------------------------------------------------ gs_altcorr_pyramid

def _grid(e, h, w, frac=(0.3, 0.6)):
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    return (torch.stack([xs + frac[0], ys + frac[1]], -1)[None].repeat(e, 1, 1, 1)).contiguous()


def _altcorr_case(case):
    """(feature maps [1,N,128,H,W], coords [1,E,H,W,2], ii, jj).  Inside one 4 x 4 tile the window origins
    floor(coords) - 3 of an identity map span 3; moving the tile's LAST column (row) pixel by +5 px makes the spread exactly
    8 (a 16-wide box: matrix-core path), +6 px exactly 9 (per-pixel path); halved coordinates put levels 1-3 of the same
    wave back on the matrix-core path."""
    g = torch.Generator().manual_seed(910 + len(case))
    if case == "ragged 10x14, nine edges":
        h, w = 10, 14
        fm = (1.5 * torch.randn(1, 5, 128, h, w, generator=g)).half()
        ii, jj = torch.tensor([0, 1, 2, 4, 3, 1, 0, 2, 4]), torch.tensor([1, 0, 4, 2, 3, 3, 4, 0, 1])
        coords = _grid(9, h, w) + 3.0 * torch.randn(9, h, w, 2, generator=g)
        return fm, coords[None].contiguous(), ii, jj
    h, w = 16, 24
    fm = (1.5 * torch.randn(1, 2, 128, h, w, generator=g)).half()
    ii, jj = torch.tensor([0, 1]), torch.tensor([1, 0])
    coords = _grid(2, h, w)
    axis, shift = (0 if " x" in case else 1), (5.0 if "spread 8" in case else 6.0)
    for e, (ty, tx) in enumerate([(0, 0), (1, 2)]):             # the moved pixel: last column (row) of tile (ty, tx)
        py, px = (4 * ty + 1, 4 * tx + 3) if axis == 0 else (4 * ty + 3, 4 * tx + 1)
        coords[e, py, px, axis] += shift
        o = torch.floor(coords[e, 4 * ty:4 * ty + 4, 4 * tx:4 * tx + 4, axis])
        assert float(o.max() - o.min()) == (8.0 if shift == 5.0 else 9.0)
    return fm, coords[None].contiguous(), ii, jj


@pytest.mark.parametrize("case", ["spread 8 in x", "spread 9 in x", "spread 8 in y", "spread 9 in y",
                                  "ragged 10x14, nine edges"])
def test_altcorr_pyramid_per_element(built_lib, case):
    """AltCorrBlock.lookup_fused = gs_altcorr_pyramid.  Reference per level: float64 dot products of the fp16 pyramid rows
    the kernel reads (0 outside the map), blended with the four weights computed in fp32 from the fp32 coordinates as
    csrc/altcorr_pyramid.hip states, one rounding; K = 128 products + 4 blend terms = 132; baseline: the same in fp32."""
    from go_slam_amd.corr import AltCorrBlock
    fm, coords, ii, jj = _altcorr_case(case)
    blk = AltCorrBlock(fm.to(DEV))
    assert blk.fused_supported(coords.to(DEV))
    out = blk.lookup_fused(coords.to(DEV), ii.to(DEV), jj.to(DEV))
    torch.cuda.synchronize()
    e, h, w = coords.shape[1:4]
    assert tuple(out.shape) == (1, e, 196, h, w) and out.dtype == torch.float16
    y = out[0].permute(0, 2, 3, 1).contiguous().cpu()
    pyr = [p[0].cpu() for p in blk.pyramid]
    ref, mag, K, base = R.altcorr_ref(pyr, coords[0], ii, jj)
    assert K == 132 and float((mag > 0).mean()) > 0.3                  # (the rest: windows of the coarse levels outside)
    _report(R.gate(y.numpy(), ref, mag, K, base, label=f"altcorr_pyramid {case}"))


# ------------------------------------------------------------------------------------------------ gs_enc_conv

# (ksize, c_in, c_out, stride): the ten layer shapes the kernel is built for (include/goslam_hip.h)
ENC_SHAPES = [(7, 4, 32, 2), (3, 32, 32, 1), (3, 32, 64, 2), (3, 64, 64, 1), (3, 64, 128, 2), (3, 128, 128, 1),
              (1, 32, 64, 2), (1, 64, 128, 2), (1, 128, 128, 1), (1, 128, 256, 1)]
# 2 x 7 x 37: stride 1 -> one full and one 5-pixel group per row, stride 2 -> 4 x 19 from odd sizes, two images;
# 1 x 9 x 70: stride 2 -> 35 outputs per row
ENC_MAPS = [(2, 7, 37), (1, 9, 70)]


def _enc_operands(regime, shape, fmap, seed):
    k, cin, cout, stride = shape
    n, h, w = fmap
    x, wt = R.operands(regime, (n, h, w, cin), (cout, cin, k, k), (k * k * cin) ** 0.5, seed=seed)
    if k == 7:                                  # the stem reads RGB0: the fourth channel and its weights are zero
        x[..., 3] = 0
        wt[:, 3] = 0
    return x, wt


def _run_enc_conv(x, wt, shape, bias16):
    """gs_enc_conv on the first c_in channels of rows c_in + 8 apart (the stem: dense, as the entry demands) into rows
    c_out + 8 apart; the 8 sentinel columns are checked"""
    from go_slam_amd import _lib
    from go_slam_amd.extractor import pack_enc_conv_weight
    k, cin, cout, stride = shape
    n, h, w, _ = x.shape
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    xs = cin if k == 7 else cin + 8
    xbuf = _strided(x, xs)
    wp = pack_enc_conv_weight((wt[:, :3] if k == 7 else wt).to(DEV))
    assert wp.numel() == _lib.lib().gs_enc_conv_wpack_elems(k, cin, cout)
    bd = None if bias16 is None else bias16.to(DEV)
    y = torch.full((n, ho, wo, cout + 8), SENTINEL, dtype=torch.float16, device=DEV)
    rc = _lib.lib().gs_enc_conv(_lib.ptr(xbuf), xs, cin, _lib.ptr(wp), _lib.ptr(bd), _lib.ptr(y), cout + 8, cout, k, stride,
                                n, h, w, None, None, _lib.stream_ptr(DEV))
    _lib.check(rc, "enc_conv")
    torch.cuda.synchronize()
    y = y.cpu()
    assert bool((y[..., cout:] == SENTINEL).all()), "the kernel wrote outside its channels"
    return y[..., :cout].contiguous()


@pytest.mark.parametrize("fmap", ENC_MAPS, ids=lambda v: "x".join(map(str, v)))
@pytest.mark.parametrize("shape", ENC_SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_enc_conv_per_element(built_lib, shape, fmap):
    """csrc/enc_conv.hip, every layer shape: fp32 accumulation and one fp16 rounding; with the fp16 bias a second rounding
    after the fp16 add (gemm_referee.conv_ref rounds where the kernel does, `two_step`, and gives the hard bound the
    allowance of gemm_referee.two_step_slack).  plain and offset on every shape, subnormal inputs on the stem and on
    3 x 3 128 -> 128."""
    k, cin, cout, stride = shape
    regimes = ["plain", "offset"] + (["subnormal"] if shape in (ENC_SHAPES[0], ENC_SHAPES[5]) else [])
    bias16 = (0.3 * torch.randn(cout, generator=torch.Generator().manual_seed(1210 + cout))).half()
    for regime in regimes:
        x, wt = _enc_operands(regime, shape, fmap, seed=1200 + 10 * k + cin + cout + fmap[2])
        if regime == "subnormal":
            assert float(x.float().max()) < 2.0 ** -14
        for bias in (None, bias16):
            ref, mag, K, base, slack = R.conv_ref(x, wt, k, stride, bias, with_slack=True)
            assert K == k * k * cin + (bias is not None)
            y = _run_enc_conv(x, wt, shape, bias)
            assert tuple(y.shape) == ref.shape
            if bias is None:
                plain_y = y
            else:           # the second rounding, exactly: the CPU's fp16 add on the kernel's own (gated) bias-free output
                assert torch.equal(y, (plain_y.float() + bias.float()).half())
            _report(R.gate(y.numpy(), ref, mag, K, base, slack=slack,
                           label=f"enc_conv {shape} {fmap} {regime} {'fp16 bias' if bias is not None else 'no bias'}"))


# ------------------------------------------------------------------------------------------------ gs_conv7x7_c4

@pytest.mark.parametrize("n,h,w,rt", [(1, 7, 9, 3), (2, 23, 37, 5)])
@pytest.mark.parametrize("relu", [False, True])
def test_conv7x7_c4_per_element(built_lib, n, h, w, rt, relu):
    """csrc/conv7x7.hip: the fp32 accumulators start at the fp32 bias, one rounding to fp16, ReLU: K = 196 + 1.  A 7 x 9
    map in strips of 3 rows (a last strip of one row, every pixel within 3 of a border) and 2 x 23 x 37 in strips of 5."""
    from go_slam_amd import _lib
    from go_slam_amd.droid_net import pack_conv7x7_c4_weight
    bias = 0.3 * torch.randn(128, generator=torch.Generator().manual_seed(1310))
    for regime in ("plain", "offset", "subnormal"):
        x, wt = R.operands(regime, (n, h, w, 4), (128, 4, 7, 7), 14.0, seed=1300 + h + w)
        ref, mag, K, base = R.conv_ref(x, wt, 7, 1, bias, relu)
        assert K == 197
        xd, wp, bd = x.to(DEV), pack_conv7x7_c4_weight(wt.to(DEV)), bias.to(DEV)
        y = torch.full((n, h, w, 128 + 8), SENTINEL, dtype=torch.float16, device=DEV)
        rc = _lib.lib().gs_conv7x7_c4(_lib.ptr(xd), _lib.ptr(wp), _lib.ptr(bd), _lib.ptr(y), 128 + 8, n, h, w, int(relu), rt,
                                      _lib.stream_ptr(DEV))
        _lib.check(rc, "conv7x7_c4")
        torch.cuda.synchronize()
        y = y.cpu()
        assert bool((y[..., 128:] == SENTINEL).all()), "the kernel wrote outside its channels"
        got = y[..., :128].contiguous().numpy()
        if relu:
            assert 0.05 < float((got == 0).mean()) < 0.95
        _report(R.gate(got, ref, mag, K, base, label=f"conv7x7_c4 {n}x{h}x{w} rt={rt} relu={int(relu)} {regime}"))
