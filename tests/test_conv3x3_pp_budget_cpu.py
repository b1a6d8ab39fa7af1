"""Register and scratch budget of conv3x3_pp_kernel, from the compiler's own report: the file is cross-compiled for gfx950
(no GPU needed, nothing is launched) and the code object's kernel metadata is read.  The kernel runs two waves per SIMD,
so every instantiation has 256 registers (VGPRs + AGPRs) and must not spill: a scratch access in the main loop would also
break its counted s_waitcnt vmcnt arithmetic."""
from kernel_metadata import kernel_metadata

# (TW, EPI, BN, PROBE) of every instantiation csrc/conv3x3_pp.hip makes; the last one only with -DGS_BUILD_PROBES
INSTANTIATIONS = [(tw, epi, bn, 0) for tw in (8, 16) for epi, bn in
                  ((0, 128), (0, 64), (1, 128), (2, 128), (3, 128), (3, 64), (4, 128))] + [(16, 0, 128, 1)]


def _kernel_metadata(tmp_path):
    return kernel_metadata("conv3x3_pp.hip", tmp_path, defines=("-DGS_BUILD_PROBES",))


def test_every_instantiation_fits_two_waves_per_simd_without_scratch(tmp_path):
    kernels = {k: v for k, v in _kernel_metadata(tmp_path).items() if "conv3x3_pp_kernel" in k}
    assert len(kernels) == len(INSTANTIATIONS), sorted(kernels)
    for tw, epi, bn, probe in INSTANTIATIONS:
        names = [k for k in kernels if f"conv3x3_pp_kernelILi{tw}ELi{epi}ELi{bn}ELb{probe}EE" in k]
        assert len(names) == 1, ((tw, epi, bn, probe), sorted(kernels))
        m = kernels[names[0]]
        print(f"TW {tw} EPI {epi} BN {bn} probe {probe}: {m}")
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (names[0], m)
        assert m["vgpr_count"] + m["agpr_count"] <= 256, (names[0], m)
