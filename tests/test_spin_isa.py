"""Build-time guard for the spin-image kernels (csrc/spin.hip): a wave keeps its 153 columns in LDS because a register array
with a run-time index would go to scratch memory, and the inverse tangent of the radial structure must fit the register budget
of four waves per SIMD beside the walk.  hipcc cross-compiles gfx950 without a GPU, so the kernels' metadata is checked on every
run of the suite.  Only the .amdhsa metadata numbers are read."""
import os
import re
import shutil
import subprocess
import sys

import pytest

from conftest import ROOT

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
sys.path.insert(0, ROOT)
from usip_amd.build import FLAGS as BUILD_FLAGS  # noqa: E402   (the ISA checked here is the ISA that ships)

FLAGS = [f for f in BUILD_FLAGS if f != "-fPIC"] + ["-S", "--cuda-device-only"]
# one u64 [153] per wave, four waves per workgroup; the structure is the template argument (0 rectangular, 1 radial)
LDS = 4 * 153 * 8
KERNELS = {"rectangular": "spin_image_kernelILi0EE", "radial": "spin_image_kernelILi1EE"}

pytestmark = pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="hipcc not present")


@pytest.fixture(scope="module")
def meta(tmp_path_factory):
    """{kernel name: {metadata key: value}} from the .amdhsa metadata"""
    out = str(tmp_path_factory.mktemp("isa") / "spin.s")
    subprocess.run([HIPCC] + FLAGS + ["-x", "hip", os.path.join(ROOT, "usip_amd", "csrc", "spin.hip"), "-o", out],
                   check=True, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=600)
    kernels = {}
    for block in open(out).read().split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        kernels[name] = {k: int(v) for k, v in re.findall(r"^    \.(\w+):\s+(\d+)\s*$", block, re.M)}
    return kernels


@pytest.mark.parametrize("structure", sorted(KERNELS))
def test_kernel_resources(meta, structure):
    found = [m for name, m in meta.items() if KERNELS[structure] in name]
    assert len(found) == 1 and len(meta) == 2, sorted(meta)            # exactly the two instantiations
    m = found[0]
    print("%s: %d VGPRs, %d SGPRs, %d B LDS" % (structure, m["vgpr_count"], m["sgpr_count"], m["group_segment_fixed_size"]))
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0
    assert m["group_segment_fixed_size"] == LDS == 4896
    assert m["vgpr_count"] <= 128                                      # 512 per SIMD lane: at least four waves per SIMD
