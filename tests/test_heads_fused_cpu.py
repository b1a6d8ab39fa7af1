"""CPU-side checks of the fused head path (gs_conv3x3_heads + gs_conv3x3_heads_finish): the packing and indexing helpers
of the Python side, and the compiler's resource report of the new kernel instantiations.  Nothing is launched here."""
import os
import re
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tap_weight_pack_stacks_the_head_images():
    from go_slam_amd.droid_net import pack_head_weight, pack_heads_tap_weights
    g = torch.Generator().manual_seed(3)
    ws = [torch.randn(2, 128, 3, 3, generator=g), torch.randn(2, 128, 3, 3, generator=g)]
    pack = pack_heads_tap_weights(ws)
    assert pack.shape == (2, 8, 64, 8) and pack.dtype == torch.float16 and pack.is_contiguous()
    for k in range(2):
        assert torch.equal(pack[k], pack_head_weight(ws[k]))
    with pytest.raises(AssertionError):
        pack_heads_tap_weights([torch.randn(1, 128, 3, 3)])


def test_workspace_shapes():
    from go_slam_amd.droid_net import heads_workspace_shapes
    assert heads_workspace_shapes(3, 13, 19, 384, 2) == ((2, 3 * 13 * 19, 18), (3, 13, 19, 128))
    assert heads_workspace_shapes(1, 13, 19, 256, 2) == ((2, 13 * 19, 18), None)       # MotionFilter.track: no agg block
    with pytest.raises(AssertionError):
        heads_workspace_shapes(1, 4, 4, 256, 3)
    with pytest.raises(AssertionError):
        heads_workspace_shapes(1, 4, 4, 320, 2)


def test_tap_products_and_gather_reproduce_the_convolution():
    """What the two kernels compute, restated on the CPU from the packed image alone: per-pixel products with the A
    fragments (lane l of k-step ks holds channels 16 ks + 8 (l >> 5) ... + 8 of column l & 31), then the gather the
    workspace's documentation states -- column (3 ky + kx) 2 + o of the neighbour at (ky - 1, kx - 1), in-image taps only
    -- equal F.conv2d with padding 1."""
    from go_slam_amd.droid_net import pack_heads_tap_weights
    g = torch.Generator().manual_seed(4)
    n, h, w = 2, 5, 7
    x = torch.randn(n, h, w, 128, generator=g).half().float()
    wt = (torch.randn(2, 128, 3, 3, generator=g) / 30).half()
    pack = pack_heads_tap_weights([wt, wt.flip(0)])[0].float()          # [8, 64, 8]
    full = pack.view(8, 2, 32, 8).permute(2, 0, 1, 3).reshape(32, 128)   # [column, channel]
    assert bool((full[18:] == 0).all())
    taps = (x.reshape(-1, 128).double() @ full[:18].double().t()).view(n, h, w, 18)
    out = torch.zeros(n, h, w, 2, dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            for r in range(h):
                for c in range(w):
                    rr, c2 = r + ky - 1, c + kx - 1
                    if 0 <= rr < h and 0 <= c2 < w:
                        out[:, r, c] += taps[:, rr, c2, (ky * 3 + kx) * 2:(ky * 3 + kx) * 2 + 2]
    ref = torch.nn.functional.conv2d(x.permute(0, 3, 1, 2).double(), wt.double(), padding=1).permute(0, 2, 3, 1)
    torch.testing.assert_close(out, ref, rtol=1e-12, atol=1e-12)


def _resource_report(src, tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "go_slam_amd", "csrc")
    out = tmp_path / "k.s"
    res = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                          "-fno-gpu-rdc", "-munsafe-fp-atomics", "-I", csrc, "-I", os.path.join(ROOT, "include"),
                          "--cuda-device-only", "-S", os.path.join(csrc, src), "-o", str(out)],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-2000:]
    pat = re.compile(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?"
                     r"\s+\.vgpr_count:\s+(\d+)")
    return {m.group(1): (int(m.group(2)), int(m.group(3))) for m in pat.finditer(open(out).read())}


def test_heads_epilogue_instantiations_have_no_scratch(tmp_path):
    """conv3x3_pp_kernel<TW, 4, 128> (the merged head convolution with the tap products in its epilogue), both tile
    widths: compiled for gfx950, no scratch, within the 256 VGPRs of two waves per SIMD -- from the code object's
    metadata, as tests/test_abi.py reads it."""
    rep = _resource_report("conv3x3_pp.hip", tmp_path)
    for tw in (8, 16):
        names = [k for k in rep if f"conv3x3_pp_kernelILi{tw}ELi4ELi128ELb0EE" in k]
        assert len(names) == 1, (tw, sorted(rep))
        scratch, vgpr = rep[names[0]]
        assert scratch == 0, f"{names[0]}: {scratch} B of scratch"
        assert vgpr <= 256, f"{names[0]}: {vgpr} VGPRs"


def test_finishing_kernel_has_no_scratch(tmp_path):
    rep = _resource_report("conv_heads.hip", tmp_path)
    names = [k for k in rep if "conv3x3_heads_finish_kernel" in k]
    assert len(names) == 1, sorted(rep)
    scratch, vgpr = rep[names[0]]
    assert scratch == 0 and vgpr <= 64, (scratch, vgpr)
