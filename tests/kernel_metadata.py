"""The compiler's own report on the kernels of one csrc/*.hip file: the file is cross-compiled for gfx950 with the
Makefile's flags (no GPU needed, nothing is launched) and the code object's kernel metadata is read."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FIELDS = ("private_segment_fixed_size", "group_segment_fixed_size", "vgpr_count", "agpr_count", "sgpr_count",
          "vgpr_spill_count", "sgpr_spill_count")


def kernel_metadata(source, tmp_path, defines=()):
    """{mangled kernel name: {field: int}} for go_slam_amd/csrc/<source>."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        assert not os.path.isdir("/opt/rocm"), "a ROCm installation is present but hipcc was not found"
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "go_slam_amd", "csrc")
    out = tmp_path / (os.path.splitext(source)[0] + ".s")
    res = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                          "-fno-gpu-rdc", "-munsafe-fp-atomics", *defines, "-I", csrc, "-I",
                          os.path.join(ROOT, "include"), "--cuda-device-only", "-S",
                          os.path.join(csrc, source), "-o", str(out)],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-2000:]
    text = open(out).read()
    meta = text[text.index("amdhsa.kernels:"):]
    kernels = {}
    for block in re.split(r"\n  - (?=\.)", meta)[1:]:                    # one YAML list item per kernel
        field = lambda key: re.search(rf"^\s*\.{key}:\s+(\S+)\s*$", block, re.M)
        kernels[field("name").group(1)] = {k: int(field(k).group(1)) for k in FIELDS if field(k)}
    return kernels
