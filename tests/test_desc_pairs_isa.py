"""Build-time guard for the two pair builders' kernels (csrc/desc_pairs.hip, csrc/pairs.hip, both instantiating
csrc/cloud_stage.h): the per-pair draws (24 float64 parameters), the float64 tables' rotation products and the per-slot
augmentation live in registers with compile-time indices only.  If an index became dynamic, or the register budget were exceeded, they would move to scratch memory;
hipcc cross-compiles gfx950 without a GPU, so the ISA is checked here on every run of the suite."""
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


def compile_asm(tmp_path_factory, unit):
    out = str(tmp_path_factory.mktemp("isa") / (unit + ".s"))
    subprocess.run([HIPCC] + FLAGS + ["-x", "hip", os.path.join(ROOT, "usip_amd", "csrc", unit + ".hip"), "-o", out],
                   check=True, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=600)
    return open(out).read()


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    return compile_asm(tmp_path_factory, "desc_pairs")


@pytest.fixture(scope="module")
def pairs_asm(tmp_path_factory):
    return compile_asm(tmp_path_factory, "pairs")


def kernels(asm):
    """{kernel name: {metadata key: value}} from the .amdhsa metadata."""
    out = {}
    for block in asm.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        out[name] = {k: int(v) for k, v in re.findall(r"^    \.(\w+):\s+(\d+)\s*$", block, re.M)}
    return out


def check_registers(asm, names):
    meta = kernels(asm)
    for want in names:
        assert sum(want in k for k in meta) == 2, sorted(meta)               # Philox and explicit draws
    assert len(meta) == 2 * len(names), sorted(meta)
    for name, m in meta.items():
        print("%s: %d VGPRs, %d SGPRs, %d B LDS" % (name, m["vgpr_count"], m["sgpr_count"], m["group_segment_fixed_size"]))
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, name
    assert "scratch_" not in asm


def test_every_kernel_stays_in_registers(asm):
    check_registers(asm, ("desc_select_kernel", "desc_mine_kernel", "cloud_points_kernel", "cloud_nodes_kernel"))    # 8


def test_every_detector_kernel_stays_in_registers(pairs_asm):
    """pairs_params_kernel draws its 24 parameters in two halves with constant indices (csrc/pairs_math.h pair_table)."""
    check_registers(pairs_asm, ("pairs_params_kernel", "cloud_points_kernel", "cloud_nodes_kernel"))                 # 6


def test_no_atomics_on_floats_and_one_integer_count(asm):
    """Every float is written by exactly one thread.  The only atomic is the workgroup's count of anchors without a
    negative candidate: an integer add in LDS (desc_mine_kernel), stored once by thread 0."""
    assert not re.search(r"\b(global|flat|ds|buffer)_(atomic_)?(add|pk_add|min|max)_(rtn_)?f(16|32|64)\b", asm)
    assert not re.search(r"\b(global|flat|buffer)_atomic", asm)
    lds_atomics = set(re.findall(r"\bds_\w*(?:add|sub|inc|min|max|and|or|xor|cmpst|wrxchg)\w*", asm))
    assert lds_atomics <= {"ds_add_u32", "ds_add_rtn_u32"}, lds_atomics


def test_detector_kernels_have_no_atomics_at_all(pairs_asm):
    assert not re.search(r"\b(global|flat|ds|buffer)_(atomic_)?(add|pk_add|min|max)_(rtn_)?f(16|32|64)\b", pairs_asm)
    assert not re.search(r"\b(global|flat|buffer)_atomic", pairs_asm)
    assert not re.findall(r"\bds_\w*(?:add|sub|inc|min|max|and|or|xor|cmpst|wrxchg)\w*", pairs_asm)
