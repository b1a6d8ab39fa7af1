"""gs_conv3x3_pp and its fused epilogues on 16x16x32 MFMAs: which lane holds which pixel and channel is checked EXACTLY
with one-hot weights (every output element is one input element, so a wrong lane <-> pixel or lane <-> channel mapping in
the fragment reads or in the accumulator scatter moves values instead of perturbing them), then the same shapes with
random operands, and the gate / head epilogues against the unfused kernels they replace."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

# (n, h, w, C, n_out, tw): tiles spanning images, partial tiles in x and at the batch end, one chunk and two chunks, both
# tile widths, 64-channel workgroups (n_out = 64), two channel blocks (n_out = 256)
SHAPES = [(2, 5, 19, 32, 128, 16), (3, 7, 9, 64, 256, 8), (2, 33, 16, 32, 64, 16)]


def _run_pp(x, wt, n_out, tw, xcd):
    from go_slam_amd import _lib
    from go_slam_amd.droid_net import pack_conv3x3_weight
    n, h, w, c = x.shape
    wp = pack_conv3x3_weight(wt, 32)
    y = torch.full((n, h, w, n_out + 8), 7.0, dtype=torch.float16, device=DEV)
    rc = _lib.lib().gs_conv3x3_pp(_lib.ptr(x), c, c, _lib.ptr(wp), tw, _lib.ptr(y), n_out + 8, n_out, n, h, w, xcd,
                                  _lib.stream_ptr(DEV))
    _lib.check(rc, "conv3x3_pp")
    assert bool((y[..., n_out:] == 7.0).all()), "the kernel wrote outside its channels"
    return y[..., :n_out]


@pytest.mark.parametrize("n,h,w,c,n_out,tw", SHAPES)
def test_one_hot_weights_place_every_element_exactly(built_lib, n, h, w, c, n_out, tw):
    """output channel o = input channel (7 o) % C at tap o % 9: integer-valued fp16 input, so every product and sum is
    exact and the output must EQUAL the shifted input slices."""
    g = torch.Generator().manual_seed(17 * n + w)
    x = torch.randint(-64, 65, (n, h, w, c), generator=g).half()
    wt = torch.zeros(n_out, c, 3, 3)
    want = torch.empty(n, h, w, n_out)
    xp = torch.nn.functional.pad(x.float(), (0, 0, 1, 1, 1, 1))          # zero border of one pixel in y and x
    for o in range(n_out):
        ci, ky, kx = (o * 7) % c, (o % 9) // 3, (o % 9) % 3
        wt[o, ci, ky, kx] = 1.0
        want[..., o] = xp[:, ky:ky + h, kx:kx + w, ci]
    for xcd in (0, 1):
        got = _run_pp(x.to(DEV), wt.half().to(DEV), n_out, tw, xcd).float().cpu()
        bad = (got != want)
        assert torch.equal(got, want), f"xcd={xcd}: {int(bad.sum())} of {want.numel()} elements, first at " \
                                       f"{bad.nonzero()[0].tolist() if bool(bad.any()) else None}"


@pytest.mark.parametrize("n,h,w,c,n_out,tw", SHAPES)
def test_random_operands_match_fp32_convolution_and_repeat_bit_for_bit(built_lib, n, h, w, c, n_out, tw):
    """the same shapes against F.conv2d in fp32 on the same fp16 operands (the tolerance test_widen_gpu.py uses for this
    kernel), four runs over both workgroup orders: loads stay in flight across barriers, a staging race shows as
    run-to-run differences."""
    g = torch.Generator().manual_seed(n * 1000 + c + w)
    x = torch.randn(n, h, w, c, generator=g).half().to(DEV)
    wt = (torch.randn(n_out, c, 3, 3, generator=g) / (3.0 * c ** 0.5)).half().to(DEV)
    ref = torch.nn.functional.conv2d(x.permute(0, 3, 1, 2).float(), wt.float(), padding=1).permute(0, 2, 3, 1)
    first = None
    for rep in range(4):
        y = _run_pp(x, wt, n_out, tw, rep & 1)
        torch.testing.assert_close(y.float(), ref, rtol=2e-3, atol=2e-3)
        if first is None:
            first = y.clone()
        else:
            assert torch.equal(y, first), f"run {rep} differs from run 0"


def test_gate_epilogues_equal_convolution_plus_gate_kernels(built_lib):
    """gs_conv3x3_gru_zr2 / gs_conv3x3_gru_q against gs_conv3x3_pp followed by gs_gru_gate_zr / gs_gru_gate_q on the same
    operands at (n, h, w) = (2, 9, 20): one accumulation order across the epilogue variants, same rounding points.  The
    bound is the one test_fused_gru_epilogues_equal_conv_plus_gate_kernels states: at most one fp16 ulp of a value below 1
    (2^-11) on at most 1 element in 10^4."""
    from go_slam_amd import _lib
    from go_slam_amd.droid_net import conv3x3_pp_tile_width, pack_conv3x3_weight
    L, st = _lib.lib(), _lib.stream_ptr(DEV)
    n, h, w, c_rest = 2, 9, 20, 192
    hw, cin = h * w, 128 + c_rest
    g = torch.Generator().manual_seed(23)
    dev16 = lambda t: t.half().to(DEV).contiguous()
    net = dev16(torch.tanh(torch.randn(n, hw, 128, generator=g)))
    xr = dev16(torch.relu(torch.randn(n, hw, c_rest, generator=g)))
    inp_pre = dev16(0.5 * torch.randn(n, hw, 384, generator=g))
    wzr = pack_conv3x3_weight((torch.randn(256, cin, 3, 3, generator=g) / (3.0 * cin ** 0.5)).half().to(DEV))
    wq = pack_conv3x3_weight((torch.randn(128, cin, 3, 3, generator=g) / (3.0 * cin ** 0.5)).half().to(DEV))
    bzr, gzr = (0.3 * torch.randn(256, generator=g)).to(DEV), (0.3 * torch.randn(n, 256, generator=g)).to(DEV)
    bq, gq = (0.3 * torch.randn(128, generator=g)).to(DEV), (0.3 * torch.randn(n, 128, generator=g)).to(DEV)
    z1 = torch.empty(n, hw, 128, dtype=torch.float16, device=DEV)
    rn1, out1, z2, out2 = (torch.empty_like(z1) for _ in range(4))
    _lib.check(L.gs_conv3x3_gru_zr2(_lib.ptr(net), _lib.ptr(xr), c_rest, c_rest, _lib.ptr(wzr), _lib.ptr(bzr),
                                    _lib.ptr(gzr), _lib.ptr(inp_pre), _lib.ptr(z1), _lib.ptr(rn1), n, h, w, st), "zr2")
    _lib.check(L.gs_conv3x3_gru_q(_lib.ptr(rn1), _lib.ptr(xr), c_rest, c_rest, _lib.ptr(wq), _lib.ptr(bq), _lib.ptr(gq),
                                  _lib.ptr(inp_pre), _lib.ptr(z1), _lib.ptr(net), _lib.ptr(out1), n, h, w, st), "q")
    hx = torch.cat([net, xr], -1).contiguous()
    zr_pre = torch.empty(n, hw, 256, dtype=torch.float16, device=DEV)
    q_pre = torch.empty(n, hw, 128, dtype=torch.float16, device=DEV)
    tw = conv3x3_pp_tile_width(w)
    _lib.check(L.gs_conv3x3_pp(_lib.ptr(hx), cin, cin, _lib.ptr(wzr), tw, _lib.ptr(zr_pre), 256, 256, n, h, w, 0, st), "pp")
    _lib.check(L.gs_gru_gate_zr(_lib.ptr(zr_pre), _lib.ptr(bzr), _lib.ptr(gzr), _lib.ptr(inp_pre), _lib.ptr(hx),
                                _lib.ptr(z2), n, hw, cin, st), "gate zr")
    _lib.check(L.gs_conv3x3_pp(_lib.ptr(hx), cin, cin, _lib.ptr(wq), tw, _lib.ptr(q_pre), 128, 128, n, h, w, 0, st), "pp")
    _lib.check(L.gs_gru_gate_q(_lib.ptr(q_pre), _lib.ptr(bq), _lib.ptr(gq), _lib.ptr(inp_pre), _lib.ptr(z2),
                               _lib.ptr(net), _lib.ptr(out2), n, hw, st), "gate q")
    torch.cuda.synchronize()
    assert float(out2.float().std()) > 0.05 and float(z2.float().std()) > 0.05          # the referee computes something
    for name, a, b in (("z", z1, z2), ("r * net", rn1, hx[..., :128]), ("net_out", out1, out2)):
        assert torch.isfinite(a.float()).all(), name
        d = (a.float() - b.float()).abs()
        print(f"{name}: max |diff| {float(d.max()):.3e}, {int((d > 0).sum())} of {a.numel()} elements differ")
        assert float(d.max()) <= 2.0 ** -11 and int((d > 0).sum()) <= a.numel() // 10000, \
            (name, float(d.max()), int((d > 0).sum()))


@pytest.mark.parametrize("tw", [8, 16])
def test_fused_heads_equal_convolution_plus_head_kernel(built_lib, tw):
    """the merged head convolution with the tap products in its epilogue (gs_conv3x3_heads + gs_conv3x3_heads_finish)
    against conv_nobias (gs_conv3x3_pp, 128 -> 384) + conv3x3_head twice at (n, h, w) = (2, 9, 20): EQUAL, as are the
    trailing 128 channels both routes store."""
    import go_slam_amd.droid_net as DN
    n, h, w, n_out = 2, 9, 20, 384
    g = torch.Generator().manual_seed(31)
    net = torch.tanh(torch.randn(n, 128, h, w, generator=g)).half().to(DEV).contiguous(memory_format=torch.channels_last)
    wt = (torch.randn(n_out, 128, 3, 3, generator=g) / (3.0 * 128 ** 0.5)).half().to(DEV)
    wt = wt.contiguous(memory_format=torch.channels_last)
    in_bias = [(0.3 * torch.randn(128, generator=g)).to(DEV) for _ in range(3)]
    convs = []
    for _ in range(2):
        conv = torch.nn.Conv2d(128, 2, 3, padding=1)
        with torch.no_grad():
            conv.weight.copy_(torch.randn(2, 128, 3, 3, generator=g) / 12.0)
            conv.bias.copy_(torch.randn(2, generator=g))
        convs.append(conv.to(DEV))
    keep = DN.CONV3X3_IMPL
    try:
        DN.CONV3X3_IMPL = "own"
        heads = DN.conv_nobias(net, wt, 1, 1) if tw == DN.conv3x3_pp_tile_width(w) else DN.conv3x3_hip(net, wt, tw)
    finally:
        DN.CONV3X3_IMPL = keep
    cache = DN.WeightPacks()
    delta_ref = DN.conv3x3_head(heads, convs[0], cache, "none", in_channel=0, in_bias=in_bias[0], in_relu=True)
    weight_ref = DN.conv3x3_head(heads, convs[1], cache, "sigmoid", in_channel=128, in_bias=in_bias[1], in_relu=True)
    ts, rs = DN.heads_workspace_shapes(n, h, w, n_out, 2)
    taps = torch.full(ts, float("nan"), dtype=torch.float32, device=DEV)
    rest = torch.full((n, rs[3], h, w), float("nan"), dtype=torch.float16, device=DEV).contiguous(
        memory_format=torch.channels_last)
    tapw = DN.pack_heads_tap_weights([conv.weight for conv in convs])
    b0, b1 = (conv.bias.detach().float().contiguous() for conv in convs)
    delta, weight = DN.conv3x3_heads_fused(net, wt, tapw, torch.cat(in_bias[:2]).contiguous(), taps, rest, b0, b1, tw=tw)
    torch.cuda.synchronize()
    assert float(delta_ref.abs().max()) > 0.1 and float(weight_ref.std()) > 0.01
    assert torch.equal(delta, delta_ref), int((delta != delta_ref).sum())
    assert torch.equal(weight, weight_ref), int((weight != weight_ref).sum())
    assert torch.equal(rest.permute(0, 2, 3, 1), heads.permute(0, 2, 3, 1)[..., 256:384])
