"""Build-time guard for the SIFT3D kernels (csrc/sift.hip): a lane keeps its 2 S scale-space sums, its 25-entry neighbour list
(25 float64 distances and 25 int32 rows) or its 2 (S - 1) minima and maxima in registers.  If an index became dynamic, or the
register budget were exceeded, they would move to scratch memory; hipcc cross-compiles gfx950 without a GPU, so the kernels'
metadata is checked on every run of the suite.  Only the .amdhsa metadata numbers are read."""
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
SCALES = range(4, 12)                                                  # S = n_scales_per_octave + 3: one instantiation each
# the scale space stages two tiles of 256 16-byte rows; the 25-list kernel adds the tiles' original rows (two
# tiles of 256 int32) and four float64 slots of the workgroup-wide maximum; the voxel average keeps three counts per wave
LDS = {"sift_voxel_keys_kernel": 0, "sift_voxel_average_kernel": 3 * 4 * 4, "sift_dog_kernel": 2 * 256 * 16,
       "sift_nearest_kernel": 2 * 256 * 16 + 2 * 256 * 4 + 4 * 8, "sift_extrema_kernel": 0}
VGPRS = {"sift_voxel_keys_kernel": 128, "sift_voxel_average_kernel": 128, "sift_dog_kernel": 128, "sift_nearest_kernel": 256,
         "sift_extrema_kernel": 128}
COPIES = {"sift_dog_kernel": len(SCALES), "sift_extrema_kernel": len(SCALES)}

pytestmark = pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="hipcc not present")


@pytest.fixture(scope="module")
def meta(tmp_path_factory):
    """{kernel name: {metadata key: value}} from the .amdhsa metadata"""
    out = str(tmp_path_factory.mktemp("isa") / "sift.s")
    subprocess.run([HIPCC] + FLAGS + ["-x", "hip", os.path.join(ROOT, "usip_amd", "csrc", "sift.hip"), "-o", out],
                   check=True, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=600)
    kernels = {}
    for block in open(out).read().split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        kernels[name] = {k: int(v) for k, v in re.findall(r"^    \.(\w+):\s+(\d+)\s*$", block, re.M)}
    return kernels


@pytest.mark.parametrize("kernel", sorted(LDS))
def test_kernel_resources(meta, kernel):
    found = {name: m for name, m in meta.items() if kernel in name}
    assert len(found) == COPIES.get(kernel, 1) and len(meta) == 3 + 2 * len(SCALES), sorted(meta)
    for name, m in sorted(found.items()):
        print("%s: %d VGPRs, %d SGPRs, %d B LDS" % (name, m["vgpr_count"], m["sgpr_count"], m["group_segment_fixed_size"]))
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0
        assert m["group_segment_fixed_size"] == LDS[kernel]
        assert m["vgpr_count"] <= VGPRS[kernel]                         # 128: at least four waves per SIMD; 256: two
