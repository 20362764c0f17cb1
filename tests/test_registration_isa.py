"""Build-time guard for the RANSAC trial kernel (csrc/registration.hip): one lane per trial keeps a 4x4 Jacobi eigen-solve
in float64 registers -- two 4x4 arrays indexed by compile-time constants only.  If an index became dynamic, or the register
budget were exceeded, the arrays would move to scratch memory and every rotation would go through it; hipcc
cross-compiles gfx950 without a GPU, so the ISA is checked here on every run of the suite."""
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
    out = str(tmp_path_factory.mktemp("isa") / "registration.s")
    subprocess.run([HIPCC] + FLAGS + ["-x", "hip", os.path.join(ROOT, "usip_amd", "csrc", "registration.hip"), "-o", out],
                   check=True, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=600)
    return open(out).read()


def kernels(asm):
    """{kernel name: {metadata key: value}} from the .amdhsa metadata."""
    out = {}
    for block in asm.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        out[name] = {k: int(v) for k, v in re.findall(r"^    \.(\w+):\s+(\d+)\s*$", block, re.M)}
    return out


def test_trial_kernels_keep_the_eigen_solve_in_registers(asm):
    meta = {k: v for k, v in kernels(asm).items() if "ransac_trials_kernel" in k}
    assert len(meta) == 2, sorted(meta)                                  # Philox and explicit draws
    for name, m in meta.items():
        print("%s: %d VGPRs, %d SGPRs, %d B LDS" % (name, m["vgpr_count"], m["sgpr_count"], m["group_segment_fixed_size"]))
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, name
        assert m["vgpr_count"] <= 128, name                               # 106 / 108 as built: four waves per SIMD
        assert m["group_segment_fixed_size"] == 6 * 1024 * 4, name        # the pair's coordinates, float32
    body = asm[asm.index("ransac_trials_kernel"):]
    assert "scratch_" not in body[:body.index(".Lfunc_end")]


def test_no_new_kernel_uses_scratch_or_float_atomics(asm):
    for name, m in kernels(asm).items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, name
    assert not re.search(r"\b(global|flat|ds)_(atomic_)?(add|pk_add)_(rtn_)?f(32|64)\b", asm)   # sums in a fixed order only
