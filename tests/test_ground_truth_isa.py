"""Build-time guard for the f-18 kernels (csrc/ground_truth.hip): a lane of the reach walk keeps its moved row, its least d2
and the pose in registers, a lane of the information sum its ten sums.  If an index became dynamic, or the register budget were
exceeded, they would move to scratch memory; hipcc cross-compiles gfx950 without a GPU, so the kernels' metadata is checked on
every run of the suite.  Only the .amdhsa metadata numbers are read."""
import os
import re
import shutil
import subprocess
import sys

import pytest

from conftest import ROOT

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
sys.path.insert(0, ROOT)
from usip_amd import ground_truth  # noqa: E402,F401   (the Python surface the kernels are reached through)
from usip_amd.build import FLAGS as BUILD_FLAGS  # noqa: E402   (the ISA checked here is the ISA that ships)

FLAGS = [f for f in BUILD_FLAGS if f != "-fPIC"] + ["-S", "--cuda-device-only"]
# DESIGN 8n.  reach: two tiles of 256 rows as three float64 each, Rt[12], the four waves' smallest and largest x, and 256 B
# the compiler adds for the barrier reductions (__syncthreads_or, __syncthreads_count).  information: 256 lanes of ten float64
# partial sums (registration_math.h's tree_sum) and Rt[12].
LDS = {"gt_reach_kernel": 2 * 3 * 256 * 8 + 96 + 64 + 256,
       "gt_ratio_kernel": 0,
       "gt_information_kernel": 256 * 10 * 8 + 96}
SLACK = 64                                                             # alignment padding between the arrays
# as built: reach 74, ratio 20, information 66; the walk stays at six waves per SIMD up to 80 registers a lane
VGPRS = {"gt_reach_kernel": 80, "gt_ratio_kernel": 24, "gt_information_kernel": 72}

pytestmark = pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="hipcc not present")


@pytest.fixture(scope="module")
def meta(tmp_path_factory):
    """[(kernel name, {metadata key: value})] from the .amdhsa metadata"""
    out = str(tmp_path_factory.mktemp("isa") / "ground_truth.s")
    subprocess.run([HIPCC] + FLAGS + ["-x", "hip", os.path.join(ROOT, "usip_amd", "csrc", "ground_truth.hip"), "-o", out],
                   check=True, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=600)
    kernels = []
    for block in open(out).read().split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        kernels.append((name, {k: int(v) for k, v in re.findall(r"^    \.(\w+):\s+(\d+)\s*$", block, re.M)}))
    return kernels


@pytest.mark.parametrize("kernel", sorted(LDS))
def test_kernel_resources(meta, kernel):
    found = [m for name, m in meta if kernel in name]
    assert len(found) == 1 and len(meta) == len(LDS), [name for name, _ in meta]
    m = found[0]
    print("%s: %d VGPRs, %d SGPRs, %d B LDS" % (kernel, m["vgpr_count"], m["sgpr_count"], m["group_segment_fixed_size"]))
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0
    assert LDS[kernel] <= m["group_segment_fixed_size"] <= LDS[kernel] + SLACK
    assert m["vgpr_count"] <= VGPRS[kernel]
