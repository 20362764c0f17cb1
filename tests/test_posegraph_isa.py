"""Build-time guard for the f-14 kernels (csrc/posegraph.hip): a lane of the optimiser keeps an edge's 6 x 6 matrices, the
three running values of its rows of the system and its fragment's pose in registers, a lane of the information kernel its
nine sums.  If an index became dynamic, or the register budget were exceeded, they would move to scratch memory; hipcc
cross-compiles gfx950 without a GPU, so the kernels' metadata is checked on every run of the suite.  Only the .amdhsa
metadata numbers are read."""
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
# DESIGN 8j.  information: 256 lanes of ten float64 partial sums (registration_math.h's tree_sum).  posegraph: the right-hand
# side and the solution, 768 float64 each; the pivot; the 129 starts of the incidence lists; the scene's sixteen pointers, two
# scalars and five integers (168 B); and 256 B the compiler adds for the barrier reductions (__syncthreads_or).
LDS = {"icp_information_kernel": 256 * 10 * 8,
       "posegraph_kernel": 2 * 768 * 8 + 8 + 129 * 4 + 168 + 256}
SLACK = 64                                                             # alignment padding between the arrays
# as built: information 46, posegraph 267 (one workgroup of four waves per scene: a wave may take all 512 of its SIMD); a few
# registers of room each, so that neither can double unnoticed
VGPRS = {"icp_information_kernel": 56, "posegraph_kernel": 280}

pytestmark = pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="hipcc not present")


@pytest.fixture(scope="module")
def meta(tmp_path_factory):
    """[(kernel name, {metadata key: value})] from the .amdhsa metadata"""
    out = str(tmp_path_factory.mktemp("isa") / "posegraph.s")
    subprocess.run([HIPCC] + FLAGS + ["-x", "hip", os.path.join(ROOT, "usip_amd", "csrc", "posegraph.hip"), "-o", out],
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
