"""The flow-revision and confidence heads finished inside the merged head convolution (gs_conv3x3_heads +
gs_conv3x3_heads_finish) against the three-launch route they replace on the same operands: gs_conv3x3_pp 128 -> 384 into a
384-wide tensor, then gs_conv3x3_head twice.  Same operand arithmetic, same MFMA accumulation chain, same gather order and
epilogue expressions: every comparison here is for EQUALITY, bit for bit."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _operands(n, h, w, n_out, seed):
    g = torch.Generator().manual_seed(seed)
    net = torch.tanh(torch.randn(n, 128, h, w, generator=g)).half().to(DEV).contiguous(memory_format=torch.channels_last)
    wt = (torch.randn(n_out, 128, 3, 3, generator=g) / (3.0 * 128 ** 0.5)).half().to(DEV)
    wt = wt.contiguous(memory_format=torch.channels_last)
    in_bias = [(0.3 * torch.randn(128, generator=g)).to(DEV) for _ in range(n_out // 128)]
    convs = []
    for _ in range(2):
        c = torch.nn.Conv2d(128, 2, 3, padding=1)
        with torch.no_grad():
            c.weight.copy_(torch.randn(2, 128, 3, 3, generator=g) / 12.0)
            c.bias.copy_(torch.randn(2, generator=g))
        convs.append(c.to(DEV))
    return net, wt, in_bias, convs


def _three_launch_route(net, wt, in_bias, convs, tw):
    import go_slam_amd.droid_net as DN
    heads = DN.conv3x3_hip(net, wt, tw)
    cache = DN.WeightPacks()
    delta = DN.conv3x3_head(heads, convs[0], cache, "none", in_channel=0, in_bias=in_bias[0], in_relu=True)
    weight = DN.conv3x3_head(heads, convs[1], cache, "sigmoid", in_channel=128, in_bias=in_bias[1], in_relu=True)
    return heads, delta, weight


def _fused_route(net, wt, in_bias, convs, tw, fill):
    import go_slam_amd.droid_net as DN
    n, _, h, w = net.shape
    ts, rs = DN.heads_workspace_shapes(n, h, w, wt.shape[0], 2)
    taps = torch.full(ts, fill, dtype=torch.float32, device=DEV)        # every element the finish reads must be written
    rest = None
    if rs is not None:
        rest = torch.full((n, rs[3], h, w), fill, dtype=torch.float16, device=DEV).contiguous(
            memory_format=torch.channels_last)
    tapw = DN.pack_heads_tap_weights([c.weight for c in convs])
    tapb = torch.cat(in_bias[:2]).contiguous()
    b0, b1 = (c.bias.detach().float().contiguous() for c in convs)
    delta, weight = DN.conv3x3_heads_fused(net, wt, tapw, tapb, taps, rest, b0, b1, tw=tw)
    return rest, delta, weight


# (n, h, w, merged channels, tile width; None = the launcher's choice)
#  (3, 13, 19) at tw 16: 39 stacked rows -> a 512-pixel tile across two image boundaries + a partial second row tile, a
#              partial second column tile; at tw 8: 64-row tiles, three column tiles
#  (2, 5, 7):  everything inside one partial tile
#  (2, 9, 8):  w <= 8, the launcher itself picks the 8-wide instantiation
#  (1, 13, 19) with 256 channels: the `ii is None` form (MotionFilter.track), no trailing block, y = NULL
CASES = [(3, 13, 19, 384, 16), (3, 13, 19, 384, 8), (2, 5, 7, 384, 16), (2, 5, 7, 384, 8), (2, 9, 8, 384, None),
         (1, 13, 19, 256, 16), (1, 13, 19, 256, 8), (1, 13, 19, 256, None)]


@pytest.mark.parametrize("n,h,w,n_out,tw", CASES)
def test_fused_heads_equal_conv_plus_head_kernels(built_lib, n, h, w, n_out, tw):
    import go_slam_amd.droid_net as DN
    if tw is None:
        assert DN.conv3x3_pp_tile_width(w) == 8
    net, wt, in_bias, convs = _operands(n, h, w, n_out, seed=100 * n + w)
    heads, delta_ref, weight_ref = _three_launch_route(net, wt, in_bias, convs, tw)
    torch.cuda.synchronize()
    assert float(delta_ref.abs().max()) > 0.1 and float(weight_ref.std()) > 0.01       # the referee computes something
    for fill in (float("nan"), 7.0):                                   # twice, over differently poisoned workspaces
        rest, delta, weight = _fused_route(net, wt, in_bias, convs, tw, fill)
        torch.cuda.synchronize()
        print(f"n={n} h={h} w={w} n_out={n_out} tw={tw}: delta differs in {int((delta != delta_ref).sum())}, weight in "
              f"{int((weight != weight_ref).sum())} of {delta.numel()} elements")
        assert torch.equal(delta, delta_ref)
        assert torch.equal(weight, weight_ref)
        if n_out == 384:
            got = rest.permute(0, 2, 3, 1)
            assert got.is_contiguous() and torch.equal(got, heads.permute(0, 2, 3, 1)[..., 256:384])
        else:
            assert rest is None


def test_update_operator_outputs_equal_with_and_without_fused_heads(built_lib):
    """A whole UpdateModule call at (n, h, w) = (3, 13, 19): net, delta, weight, eta and the upsampling mask under
    FUSE_HEAD_TAPS on and off are EQUAL (the GraphAgg branch reads the compact agg.conv1 block on one side and the slice
    of the 384-wide tensor on the other)."""
    import go_slam_amd.droid_net as DN
    torch.manual_seed(41)
    op = DN.UpdateModule().to(DEV).eval().to(memory_format=torch.channels_last)
    E, h, w = 3, 13, 19
    g = torch.Generator().manual_seed(42)
    cl = lambda t: t.half().to(DEV).contiguous(memory_format=torch.channels_last).unsqueeze(0)
    net = cl(torch.tanh(torch.randn(E, 128, h, w, generator=g)))
    inp = cl(torch.relu(torch.randn(E, 128, h, w, generator=g)))
    corr = cl(0.5 * torch.randn(E, 196, h, w, generator=g))
    flow = torch.randn(1, E, 4, h, w, generator=g).to(DEV)
    ii = torch.tensor([0, 0, 1], device=DEV)
    keep = (DN.CONV3X3_IMPL, DN.FUSE_HEAD_TAPS)
    out = {}
    try:
        DN.CONV3X3_IMPL = "own"
        for fused in (False, True, True):                              # the second fused call reuses the workspaces
            DN.FUSE_HEAD_TAPS = fused
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
                res = op(net.clone(), inp, corr, flow, ii, ii)
            out[fused] = [res[0], res[1], res[2], res[3], res[4].materialize().clone()]
            if fused:
                assert set(op._heads_ws) == {(E, h, w, 384, net.device)}
    finally:
        DN.CONV3X3_IMPL, DN.FUSE_HEAD_TAPS = keep
    assert not hasattr(out[True][1], "materialize") and out[True][1].shape == (1, E, h, w, 2)
    for a, b, name in zip(out[True], out[False], ("net", "delta", "weight", "eta", "upmask")):
        assert torch.isfinite(a.float()).all(), name
        assert torch.equal(a, b), f"{name}: {int((a != b).sum())} of {a.numel()} elements differ"
