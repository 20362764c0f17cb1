"""Build-time guard for the f-9 kernels (csrc/fragments.hip), in the pattern of tests/test_registration_isa.py: the large
RANSAC trial kernel keeps csrc/registration.hip's eigen-solve in registers and stages ONE chunk of correspondences in LDS
(not the largest pair), the top-k lists stay in registers, and nothing adds floats atomically.  hipcc cross-compiles
gfx950 without a GPU, so the ISA is checked on every run of the suite."""
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
CHUNK = 1024                                        # csrc/fragments_math.h

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


def test_header_and_test_agree_on_the_chunk():
    text = open(os.path.join(ROOT, "usip_amd", "csrc", "fragments_math.h")).read()
    assert int(re.search(r"constexpr int CHUNK = (\d+);", text).group(1)) == CHUNK
    assert int(re.search(r"constexpr int NMAX_LARGE = (\d+);", text).group(1)) == 10240


def test_large_trial_kernels_stage_one_chunk_and_keep_four_waves(asm):
    meta = {k: v for k, v in kernels(asm).items() if "ransac_trials_large_kernel" in k}
    assert len(meta) == 2, sorted(meta)                                  # Philox and explicit draws
    for name, m in meta.items():
        print("%s: %d VGPRs, %d SGPRs, %d B LDS" % (name, m["vgpr_count"], m["sgpr_count"], m["group_segment_fixed_size"]))
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, name
        assert m["vgpr_count"] <= 128, name                               # 112 as built: four waves per SIMD
        assert m["group_segment_fixed_size"] == 6 * CHUNK * 4, name       # one chunk, not 6 * 10240 * 4
    body = asm[asm.index("ransac_trials_large_kernel"):]
    assert "scratch_" not in body[:body.index(".Lfunc_end")]


def test_select_kernel_keeps_no_flags_per_correspondence(asm):
    meta = {k: v for k, v in kernels(asm).items() if "ransac_select_large_kernel" in k}
    assert len(meta) == 2, sorted(meta)
    for name, m in meta.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, name
        assert m["vgpr_count"] <= 128, name                               # 92 as built; 40 flags per lane would show


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
