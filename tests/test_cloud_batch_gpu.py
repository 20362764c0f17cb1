"""GPU test of the one check-and-launch frame of the four batch builders (usip_amd.ops.cloud_batch): apply refuses a draw
that is not in the header's layout before anything is enqueued, on each builder's fixture bank."""
import pytest
import torch

import test_desc_pairs_cpu as t_desc
import test_fragment_batch_cpu as t_frag
import test_indoor_pairs_cpu as t_indoor
from test_cloud_batch_cpu import SWAPS, smallest_case, swapped

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def device_builder(tag, case):
    """-> (the builder over the fixture's bank, the ids of the case in that bank)."""
    from usip_amd import desc_pairs, fragment_batch, indoor_pairs, pairs
    g, recipe, ids = case["g"], case["recipe"], case["ids"]
    if tag == "pairs":                                  # (Oxford refuses a bank with a scan shorter than N)
        return pairs.PairBuilder(pairs.ScanBank([case["scans"][ids[0]]], DEV), recipe, 1, DEV, mode=case["mode"]), [0]
    if tag == "desc_pairs":
        scans, poses, seq = t_desc.fixture_bank(g)
        bank = desc_pairs.PosedScanBank(scans, poses, seq, DEV, min_points=recipe.N)
        return desc_pairs.DescriptorPairBuilder(bank, recipe, len(ids), DEV, mode=case["mode"]), ids
    if tag == "indoor_pairs":
        bank = indoor_pairs.IndoorPairBank.from_arrays(t_indoor.fixture_frames(g), g["pairs"], g["icp"], DEV)
        return indoor_pairs.IndoorPairBuilder(bank, recipe, len(ids), DEV, mode=case["mode"]), ids
    return fragment_batch.FragmentBatchBuilder(fragment_batch.FragmentScanBank.from_arrays(t_frag.fixture_frames(g), DEV),
                                               recipe), ids


@pytest.mark.parametrize("tag,key", SWAPS)
def test_apply_refuses_a_draw_that_is_not_in_the_headers_layout_before_it_enqueues(tag, key):
    from usip_amd import ops
    case = smallest_case(tag)
    b, ids = device_builder(tag, case)
    out = {k: torch.full(shape, 7, dtype=dt, device=DEV)
           for k, (shape, dt) in ops.cloud_batch_table(b.spec, b.c, len(ids)).items()}
    with pytest.raises((ValueError, RuntimeError)):
        b.apply(ids, swapped(case["draws"], key), out=out)
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in out.values())
    got = b.apply(ids, case["draws"], out=out)          # the same buffers and the header's layout: written, in place
    torch.cuda.synchronize()
    assert all(got[k].data_ptr() == out[k].data_ptr() for k in out) and not bool((out[b.spec.keys[0]] == 7).all())
