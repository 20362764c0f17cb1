"""Build-time guard for the SHOT kernels (csrc/shot.hip): the frame kernel keeps its seven float64 sums, the 3x3 Jacobi and
the two axes in registers with static indices; the histogram kernel keeps a wave's 352 columns in LDS because a register array
with a run-time index would go to scratch memory.  If an index became dynamic, or the register budget were exceeded, they would
move to scratch; hipcc cross-compiles gfx950 without a GPU, so the kernels' metadata is checked on every run of the suite.  Only
the .amdhsa metadata numbers are read."""
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
# the frame kernel uses no LDS; the histogram kernel one u64 [352] per wave, four waves per workgroup
LDS = {"shot_lrf_kernel": 0, "shot_hist_kernel": 4 * 352 * 8}

pytestmark = pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="hipcc not present")


@pytest.fixture(scope="module")
def meta(tmp_path_factory):
    """{kernel name: {metadata key: value}} from the .amdhsa metadata"""
    out = str(tmp_path_factory.mktemp("isa") / "shot.s")
    subprocess.run([HIPCC] + FLAGS + ["-x", "hip", os.path.join(ROOT, "usip_amd", "csrc", "shot.hip"), "-o", out],
                   check=True, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=600)
    kernels = {}
    for block in open(out).read().split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        kernels[name] = {k: int(v) for k, v in re.findall(r"^    \.(\w+):\s+(\d+)\s*$", block, re.M)}
    return kernels


@pytest.mark.parametrize("kernel", sorted(LDS))
def test_kernel_resources(meta, kernel):
    found = [m for name, m in meta.items() if kernel in name]
    assert len(found) == 1 and len(meta) == 2, sorted(meta)
    m = found[0]
    print("%s: %d VGPRs, %d SGPRs, %d B LDS" % (kernel, m["vgpr_count"], m["sgpr_count"], m["group_segment_fixed_size"]))
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0
    assert m["group_segment_fixed_size"] == LDS[kernel]
    assert m["vgpr_count"] <= 128                                      # 512 per SIMD lane: at least four waves per SIMD
