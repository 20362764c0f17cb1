"""Build-time guard for the FGR kernels (csrc/fgr.hip): a lane keeps its 19 float64 sums, the pose and the 6 x 6 Cholesky
factor in registers.  If an index became dynamic, or the register budget were exceeded, they would move to scratch memory;
hipcc cross-compiles gfx950 without a GPU, so the kernels' metadata is checked on every run of the suite.  Only the .amdhsa
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
# DESIGN 8h.  tuples: 1024 normalised rows of six float64, the packed mutual list, norm[8], four wave totals, the fill flag.
# optimize: the same rows, 19 x 256 float64 partial sums, the 19 sums, Rt[12], 3000 16-bit row indices, the inlier count
# (the compiler pads each array to its alignment).
LDS = {"fgr_tuples_kernel": (1024 * 48 + 1024 * 4 + 64 + 16 + 4, 2),
       "fgr_optimize_kernel": (1024 * 48 + 19 * 256 * 8 + 19 * 8 + 96 + 6000 + 4, 1)}
SLACK = 64                                                             # alignment padding between the arrays
VGPRS = 128                                                            # 512 per SIMD lane: room for four waves per SIMD

pytestmark = pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="hipcc not present")


@pytest.fixture(scope="module")
def meta(tmp_path_factory):
    """[(kernel name, {metadata key: value})] from the .amdhsa metadata"""
    out = str(tmp_path_factory.mktemp("isa") / "fgr.s")
    subprocess.run([HIPCC] + FLAGS + ["-x", "hip", os.path.join(ROOT, "usip_amd", "csrc", "fgr.hip"), "-o", out],
                   check=True, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=600)
    kernels = []
    for block in open(out).read().split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        kernels.append((name, {k: int(v) for k, v in re.findall(r"^    \.(\w+):\s+(\d+)\s*$", block, re.M)}))
    return kernels


@pytest.mark.parametrize("kernel", sorted(LDS))
def test_kernel_resources(meta, kernel):
    lds, forms = LDS[kernel]
    found = [m for name, m in meta if kernel in name]
    assert len(found) == forms and len(meta) == 3, [name for name, _ in meta]     # tuples: the Philox and the explicit form
    for m in found:
        print("%s: %d VGPRs, %d SGPRs, %d B LDS" % (kernel, m["vgpr_count"], m["sgpr_count"], m["group_segment_fixed_size"]))
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0
        assert lds <= m["group_segment_fixed_size"] <= lds + SLACK
        assert m["vgpr_count"] <= VGPRS
