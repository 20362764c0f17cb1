"""Build-time guard for the FPFH kernels (csrc/fpfh.hip): the SPFH pass keeps a lane's 33 counters in LDS (bin-major, the lane
as the fast index) because a register array with a run-time index would go to scratch memory; the gather keeps 33 float64 sums
in 66 registers with static indices.  If an index became dynamic, or the register budget were exceeded, they would move to
scratch; hipcc cross-compiles gfx950 without a GPU, so the kernels' metadata is checked on every run of the suite.  Only the
.amdhsa metadata numbers are read."""
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
# two staged tiles of 256 16-byte rows, the tiles' float64 normals beside them (three planes of 256 per tile) and
# the histograms i32 [33][256]; the gather uses no LDS
LDS = {"fpfh_spfh_kernel": 2 * 256 * 16 + 2 * 3 * 256 * 8 + 33 * 256 * 4, "fpfh_gather_kernel": 0}

pytestmark = pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="hipcc not present")


@pytest.fixture(scope="module")
def meta(tmp_path_factory):
    """{kernel name: {metadata key: value}} from the .amdhsa metadata"""
    out = str(tmp_path_factory.mktemp("isa") / "fpfh.s")
    subprocess.run([HIPCC] + FLAGS + ["-x", "hip", os.path.join(ROOT, "usip_amd", "csrc", "fpfh.hip"), "-o", out],
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
