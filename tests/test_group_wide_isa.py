"""Build-time guard for the wide-group kernels (csrc/group_wide.hip): a lane keeps its NP float4s per row (and per operand) in
registers -- an array the compiler cannot index statically would go to scratch memory -- the pooling kernel uses no LDS at all
and the reduction only the 48 bytes of the block reduction (float red[3][4], csrc/bn_reduce_common.h).  hipcc cross-compiles
gfx950 without a GPU, so the kernels' metadata is checked on every run of the suite.  Only the .amdhsa metadata numbers are
read; register counts are printed (run with -s), not fixed."""
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
# the instantiations of the file, by their mangled template arguments
POOL = {"group_max_wide_kernelILi%dELb%d" % (np_, nans): (np_, nans) for np_ in (2, 3, 4) for nans in (0, 1)}
REDUCE = {"bn_bwd_reduce_wide_kernelILi%dE" % np_: np_ for np_ in (2, 3, 4)}
FINALIZE = "bn_bwd_finalize_kernel"
RED_LDS = 3 * 4 * 4

pytestmark = pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="hipcc not present")


@pytest.fixture(scope="module")
def meta(tmp_path_factory):
    """{kernel name: {metadata key: value}} from the .amdhsa metadata"""
    out = str(tmp_path_factory.mktemp("isa") / "group_wide.s")
    subprocess.run([HIPCC] + FLAGS + ["-x", "hip", os.path.join(ROOT, "usip_amd", "csrc", "group_wide.hip"), "-o", out],
                   check=True, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=600)
    kernels = {}
    for block in open(out).read().split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        kernels[name] = {k: int(v) for k, v in re.findall(r"^    \.(\w+):\s+(\d+)\s*$", block, re.M)}
    return kernels


def _one(meta, key):
    found = [m for name, m in meta.items() if key in name]
    assert len(found) == 1, (key, sorted(meta))
    return found[0]


def test_exactly_the_listed_instantiations_exist(meta):
    assert len(meta) == len(POOL) + len(REDUCE) + 1, sorted(meta)
    for key in list(POOL) + list(REDUCE) + [FINALIZE]:
        _one(meta, key)


@pytest.mark.parametrize("key", sorted(POOL))
def test_pooling_kernel_resources(meta, key):
    m = _one(meta, key)
    print("%s: %d VGPRs, %d SGPRs" % (key, m["vgpr_count"], m["sgpr_count"]))
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0
    assert m["group_segment_fixed_size"] == 0
    assert m["vgpr_count"] <= 128                                      # at least four waves per SIMD


@pytest.mark.parametrize("key", sorted(REDUCE))
def test_reduction_kernel_resources(meta, key):
    m = _one(meta, key)
    print("%s: %d VGPRs, %d SGPRs, %d B LDS" % (key, m["vgpr_count"], m["sgpr_count"], m["group_segment_fixed_size"]))
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0
    assert m["group_segment_fixed_size"] == RED_LDS == 48
    assert m["vgpr_count"] <= 128
