"""Build-time guard for the f-9 kernels (csrc/fragments.hip), in the pattern of tests/test_registration_isa.py (which holds
the RANSAC kernels both evaluations run): the top-k lists stay in registers, and nothing adds floats atomically.  hipcc
cross-compiles gfx950 without a GPU, so the ISA is checked on every run of the suite."""
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
    out = str(tmp_path_factory.mktemp("isa") / "fragments.s")
    subprocess.run([HIPCC] + FLAGS + ["-x", "hip", os.path.join(ROOT, "usip_amd", "csrc", "fragments.hip"), "-o", out],
                   check=True, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=600)
    return open(out).read()


def kernels(asm):
    """{kernel name: {metadata key: value}} from the .amdhsa metadata."""
    out = {}
    for block in asm.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        out[name] = {k: int(v) for k, v in re.findall(r"^    \.(\w+):\s+(\d+)\s*$", block, re.M)}
    return out


def test_every_kernel_is_there_and_none_uses_scratch_or_float_atomics(asm):
    meta = kernels(asm)
    for part, n in (("knn_counted_kernel", 8), ("match_union_kernel", 1), ("information_kernel", 1),
                    ("overlap_kernel", 2), ("overlap_keys_kernel", 1), ("overlap_ratio_kernel", 1)):
        assert sum(part in k for k in meta) == n, part
    for name, m in meta.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, name
    union = [m for k, m in meta.items() if "match_union_kernel" in k][0]
    assert union["group_segment_fixed_size"] <= 48 * 1024                 # 40 KB of keys and the scan
    assert not re.search(r"\b(global|flat|ds)_(atomic_)?(add|pk_add)_(rtn_)?f(32|64)\b", asm)   # sums in a fixed order only
