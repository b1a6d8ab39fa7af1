"""Register and scratch budget of the NeuS point kernels, from the compiler's own report (csrc is cross-compiled for gfx950,
nothing is launched).  Both kernels force their occupancy, and under a forced occupancy the compiler spills silently instead
of failing: neus_point_kernel runs four waves per SIMD (amdgpu_waves_per_eu(4, 4): 128 registers, and four 40 KB workgroups
fill a CU's LDS exactly), every neus_point_bwd_kernel<BINNED, AUX> two (amdgpu_waves_per_eu(2): 256 registers)."""
import pytest

from kernel_metadata import kernel_metadata


def _no_scratch(name, m):
    print(name, m)
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)


def test_neus_point_kernel_fits_four_waves_per_simd_without_scratch(tmp_path):
    kernels = kernel_metadata("neus.hip", tmp_path)
    names = [k for k in kernels if "neus_point_kernel" in k]
    assert len(names) == 1, sorted(kernels)
    m = kernels[names[0]]
    _no_scratch(names[0], m)
    assert m["vgpr_count"] + m["agpr_count"] <= 128, m
    assert m["group_segment_fixed_size"] <= 40960, m


@pytest.fixture(scope="module")
def bwd_kernels(tmp_path_factory):
    return kernel_metadata("neus_bwd.hip", tmp_path_factory.mktemp("neus_bwd"))


@pytest.mark.parametrize("binned", [0, 1])
@pytest.mark.parametrize("aux", [0, 1])
def test_neus_point_bwd_kernel_fits_two_waves_per_simd_without_scratch(bwd_kernels, binned, aux):
    names = [k for k in bwd_kernels if f"neus_point_bwd_kernelILb{binned}ELb{aux}EE" in k]
    assert len(names) == 1, sorted(bwd_kernels)
    m = bwd_kernels[names[0]]
    _no_scratch(names[0], m)
    assert m["vgpr_count"] + m["agpr_count"] <= 256, m
