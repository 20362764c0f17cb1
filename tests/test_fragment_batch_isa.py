"""Build-time guard for the evaluation fragment builder's kernels (csrc/fragment_batch.hip, the fourth unit instantiating
csrc/cloud_stage.h): compiled for gfx950 with the shipping flags, and read from the .amdhsa metadata -- three kernels times
two sources of draws, nothing in scratch, no spilled register -- and no atomic of any kind: every float is written by
exactly one thread.  hipcc cross-compiles gfx950 without a GPU, so this runs with every run of the suite."""
import re

import pytest

from test_desc_pairs_isa import compile_asm, kernels, pytestmark  # noqa: F401   (the same flags, the same skip)

NAMES = ("fragment_clouds_kernel", "cloud_points_kernel", "cloud_nodes_kernel")


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    return compile_asm(tmp_path_factory, "fragment_batch")


def test_three_kernels_times_two_draw_sources_stay_in_registers(asm):
    meta = kernels(asm)
    for want in NAMES:
        assert sum(want in k for k in meta) == 2, sorted(meta)                # Philox and explicit draws
    assert len(meta) == 2 * len(NAMES), sorted(meta)
    for name, m in meta.items():
        print("%s: %d VGPRs, %d SGPRs, %d B LDS" % (name, m["vgpr_count"], m["sgpr_count"], m["group_segment_fixed_size"]))
        assert m["private_segment_fixed_size"] == 0, name
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, name
        assert "FragmentView" in name or "fragment_clouds_kernel" in name, name    # the new instantiations, and only here


def test_no_atomics_at_all(asm):
    assert not re.search(r"\b(global|flat|buffer)_atomic", asm)
    assert not re.findall(r"\bds_\w*(?:add|sub|inc|min|max|and|or|xor|cmpst|wrxchg)\w*", asm)
