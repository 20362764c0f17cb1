"""Build-time guard for the ICP kernels (csrc/icp.hip): a lane of the walk keeps its query, its best and the pose in
registers, a lane of the fit its ten sums and the 4 x 4 Jacobi matrices.  If an index became dynamic, or the register budget
were exceeded, they would move to scratch memory; hipcc cross-compiles gfx950 without a GPU, so the kernels' metadata is
checked on every run of the suite.  Only the .amdhsa metadata numbers are read."""
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
# DESIGN 8i.  nearest: two tiles of 256 rows as three float64 and one row index each, Rt[12], the four waves' minimum x,
# and 256 B the compiler adds for the two barrier reductions (__syncthreads_or).  trim: the 256-bin histogram, four
# wave totals, the cut's row.  fit, final: 256 lanes of ten float64 partial sums (registration_math.h's tree_sum).
LDS = {"icp_init_kernel": 0,
       "icp_nearest_kernel": 2 * 3 * 256 * 8 + 2 * 256 * 4 + 96 + 32 + 256,
       "icp_trim_kernel": 256 * 4 + 16 + 4,
       "icp_fit_kernel": 256 * 10 * 8,
       "icp_final_kernel": 256 * 10 * 8}
SLACK = 64                                                             # alignment padding between the arrays
# as built: init 48, nearest 46, trim 18, fit 90, final 25; a few registers of room each, so that none can double unnoticed
# (the walk stays at ten waves per SIMD below 48 registers a lane, the fit at five below 96)
VGPRS = {"icp_init_kernel": 56, "icp_nearest_kernel": 48, "icp_trim_kernel": 24, "icp_fit_kernel": 96, "icp_final_kernel": 32}

pytestmark = pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="hipcc not present")


@pytest.fixture(scope="module")
def meta(tmp_path_factory):
    """[(kernel name, {metadata key: value})] from the .amdhsa metadata"""
    out = str(tmp_path_factory.mktemp("isa") / "icp.s")
    subprocess.run([HIPCC] + FLAGS + ["-x", "hip", os.path.join(ROOT, "usip_amd", "csrc", "icp.hip"), "-o", out],
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
