"""Build-time guard for the scan-preparation kernels (csrc/prepare.hip): the neighbour kernel keeps one K-list per lane
(K float64 distances and K int32 indices, compile-time indices only) and the normals kernel a 3x3 Jacobi eigen-solve in
float64 registers.  If an index became dynamic, or the register budget were exceeded, those arrays would move to scratch
memory; hipcc cross-compiles gfx950 without a GPU, so the ISA is checked here on every run of the suite."""
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

pytestmark = pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="hipcc not present")


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("isa") / "prepare.s")
    subprocess.run([HIPCC] + FLAGS + ["-x", "hip", os.path.join(ROOT, "usip_amd", "csrc", "prepare.hip"), "-o", out],
                   check=True, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=600)
    return open(out).read()


def kernels(asm):
    """{kernel name: {metadata key: value}} from the .amdhsa metadata."""
    out = {}
    for block in asm.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        out[name] = {k: int(v) for k, v in re.findall(r"^    \.(\w+):\s+(\d+)\s*$", block, re.M)}
    return out


def test_every_kernel_stays_in_registers(asm):
    meta = kernels(asm)
    for want in ("scan_normals_kernel", "scan_voxel_keys_kernel", "scan_voxel_average_kernel"):
        assert sum(want in k for k in meta) == 1, sorted(meta)
    assert sum("scan_knn_kernel" in k for k in meta) == 16, sorted(meta)     # K = 1 .. 16
    for name, m in meta.items():
        print("%s: %d VGPRs, %d SGPRs, %d B LDS" % (name, m["vgpr_count"], m["sgpr_count"], m["group_segment_fixed_size"]))
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, name
    assert "scratch_" not in asm
    assert not re.search(r"\b(global|flat|ds)_(atomic_)?(add|pk_add)_(rtn_)?f(32|64)\b", asm)   # sums in a fixed order only
    assert not re.search(r"\b(global|flat|ds)_atomic", asm)                                     # ... and no atomics at all


def test_neighbour_kernel_occupancy(asm):
    """at most 128 VGPRs for every K -- four waves per SIMD, i.e. four workgroups of four waves per CU, more than
    a scan's ~470 workgroups put on a CU of this chip; two staged tiles of 16-byte rows, their original indices and the four
    max slots in LDS."""
    for name, m in kernels(asm).items():
        if "scan_knn_kernel" not in name:
            continue
        assert m["vgpr_count"] <= 128, name                                   # 84 at K = 9, 127 at K = 16 as built
        assert m["group_segment_fixed_size"] == 2 * 256 * 16 + 2 * 256 * 4 + 4 * 8, name
    # the walk reads a tile row with one 16-byte LDS load, every lane at the same address
    body = asm[asm.index("scan_knn_kernelILi9E"):]
    assert "ds_read_b128" in body[:body.index(".Lfunc_end")]
