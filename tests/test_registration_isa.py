"""Build-time guard for the RANSAC kernels (csrc/registration.hip), which serve the outdoor (f-6) and the indoor (f-9)
evaluation: one lane per trial keeps a 4x4 Jacobi eigen-solve in float64 registers -- two 4x4 arrays indexed by compile-time
constants only.  If an index became dynamic, or the register budget were exceeded, the arrays would move to scratch memory
and every rotation would go through it.  The trial kernel stages ONE chunk of correspondences in LDS (not the largest pair)
and the select kernel keeps no flag per correspondence in registers.  hipcc cross-compiles gfx950 without a GPU, so the ISA
is checked here on every run of the suite."""
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
CHUNK = 1024                                        # csrc/registration_math.h

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


def test_header_and_test_agree_on_the_chunk():
    text = open(os.path.join(ROOT, "usip_amd", "csrc", "registration_math.h")).read()
    assert int(re.search(r"constexpr int CHUNK = (\d+);", text).group(1)) == CHUNK
    assert int(re.search(r"constexpr int NMAX = (\d+);", text).group(1)) == 10240


def check_trial_kernels(asm, kernel, built):
    meta = {k: v for k, v in kernels(asm).items() if kernel in k}
    assert len(meta) == 2, sorted(meta)                                  # Philox and explicit draws
    for name, m in meta.items():
        print("%s: %d VGPRs, %d SGPRs, %d B LDS" % (name, m["vgpr_count"], m["sgpr_count"], m["group_segment_fixed_size"]))
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, name
        assert m["vgpr_count"] <= 128, (name, built)                      # four waves per SIMD
        assert m["group_segment_fixed_size"] == 6 * CHUNK * 4, name       # one chunk of coordinates, float32
    body = asm[asm.index(kernel):]
    assert "scratch_" not in body[:body.index(".Lfunc_end")]


def test_trial_kernels_keep_the_eigen_solve_in_registers(asm):
    """The form for pairs of one chunk (the outdoor evaluation's): the whole pair staged once."""
    check_trial_kernels(asm, "ransac_trials_resident_kernel", "106 / 108 as built")


def test_trial_kernels_stage_one_chunk_and_keep_four_waves(asm):
    """The general form: one chunk in LDS, not 6 * 10240 * 4 bytes."""
    check_trial_kernels(asm, "ransac_trials_kernel", "112 as built")


def test_select_kernel_keeps_no_flags_per_correspondence(asm):
    meta = {k: v for k, v in kernels(asm).items() if "ransac_select_kernel" in k}
    assert len(meta) == 2, sorted(meta)
    resident = {k: v for k, v in kernels(asm).items() if "ransac_select_resident_kernel" in k}
    assert len(resident) == 2, sorted(resident)                          # pairs of one chunk: four flags per lane
    meta.update(resident)
    for name, m in meta.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, name
        assert m["vgpr_count"] <= 128, name                               # 92 as built; 40 flags per lane would show


def test_no_new_kernel_uses_scratch_or_float_atomics(asm):
    for name, m in kernels(asm).items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, name
    assert not re.search(r"\b(global|flat|ds)_(atomic_)?(add|pk_add)_(rtn_)?f(32|64)\b", asm)   # sums in a fixed order only
