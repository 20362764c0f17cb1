"""f-18 on the device: csrc/ground_truth.hip bit for bit against the host twins (cls, hits, ratio, key, info) on the tile-edge
batch, the threshold and selection cases and the seeded 4000-point scene; against getGtInfoLog.m restated in numpy on the seeded
scene; scene_ground_truth entry for entry against scene_ground_truth_cpu for every batch split; no host synchronisation."""
import numpy as np
import pytest
import torch

import ground_truth_oracle as go
from usip_amd import fragments as fr, ground_truth as gtm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def cpu(t):
    return t.cpu().numpy()


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else np.asarray(a).astype(dtype))).to(DEV)


def truth_device(bank, c, cap=gtm.CAP, seed=0, pair_ids=None):
    f1, f2, Rt = dev(c["frag1"]), dev(c["frag2"]), dev(c["Rt"])
    mask = None if c.get("mask") is None else dev(c["mask"])
    o = gtm.reach(bank, f1, f2, Rt, seed=seed, pair_ids=None if pair_ids is None else dev(pair_ids), mask=mask)
    info, order = gtm.correspondence_information(bank, f1, f2, Rt, o["key"], o["hits"], cap, want_order=True)
    out = {k: cpu(v) for k, v in o.items()}
    out["key"] = out["key"].view(np.uint64)
    out["info"], out["order"] = cpu(info), cpu(order)
    return out


def truth_host(bank, c, cap=gtm.CAP, seed=0, pair_ids=None):
    o = gtm.reach_cpu(bank, c["frag1"], c["frag2"], c["Rt"], seed=seed, pair_ids=pair_ids, mask=c.get("mask"), num_threads=16)
    o["info"], o["order"] = gtm.correspondence_information_cpu(bank, c["frag1"], c["frag2"], c["Rt"], o["key"], o["hits"], cap,
                                                               want_order=True, num_threads=16)
    return o


def same_bits(got, want, n2=None):
    for k in ("cls", "hits", "ratio", "key", "info"):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert np.array_equal(got[k].view(np.uint8) if got[k].dtype.kind == "f" else got[k],
                              want[k].view(np.uint8) if want[k].dtype.kind == "f" else want[k]), k
    if n2 is not None:                                                 # the order is compared where it is read
        for p, n in enumerate(n2):
            assert np.array_equal(got["order"][p, :n], want["order"][p, :n]), p


def scene_case(sc):
    f1, f2, trans = gtm.scene_pairs(sc["poses"])
    return dict(frag1=f1, frag2=f2, Rt=np.ascontiguousarray(trans[:, :3]))


@pytest.fixture(scope="module")
def seeded():
    sc = go.seeded_scene()
    bank = fr.FragmentBank(sc["clouds"], DEV)
    c = scene_case(sc)
    return sc, bank, c, truth_device(bank, c)


def test_tile_edge_batch_is_the_host_twin_bit_for_bit_and_alone():
    c = go.tile_edge_case()
    bank = fr.FragmentBank(c["clouds"], DEV)
    assert bank.lmax == 600
    got, want = truth_device(bank, c), truth_host(bank.host(), c)
    same_bits(got, want, np.minimum(want["hits"][:, 1], want["order"].shape[1]))
    for p in c["zero_pairs"]:
        assert not got["cls"][p].any() and not got["hits"][p].any() and not got["info"][p].any()
    assert tuple(got["hits"][26]) == (300, 300) and not got["hits"][24].any() and got["hits"][23, 1] > 0
    for p in (0, 7, 19, 23):                                           # P = 1
        one = {k: v[p:p + 1] for k, v in c.items() if k in ("frag1", "frag2", "Rt", "mask")}
        alone = truth_device(bank, one, pair_ids=np.array([p], np.int64))
        for k in ("cls", "hits", "ratio", "key", "info"):
            assert np.array_equal(alone[k][0], got[k][p]), (p, k)


def test_threshold_and_selection_cases_are_the_host_twin_bit_for_bit():
    c = go.constructed_case()
    bank = fr.FragmentBank(c["clouds"], DEV)
    ids = np.array([10, 11, 12, 13, 14], np.int64)
    for cap in (7, 300, 5000):
        got, want = truth_device(bank, c, cap, 5, ids), truth_host(bank.host(), c, cap, 5, ids)
        same_bits(got, want, np.minimum(want["hits"][:, 1], want["order"].shape[1]))
    for p in range(5):
        n2 = len(c["clouds"][c["frag2"][p]])
        assert np.array_equal(got["cls"][p, :n2], c["expect"][p]), p
    assert [int(v) for v in got["hits"][:, 1]] == list(c["near_counts"])
    got7 = truth_device(bank, c, 7, 5, ids)
    for p in range(1, 5):
        near = np.nonzero(got7["cls"][p] == 2)[0]
        want_rows = sorted(near, key=lambda r: (int(got7["key"][p, r]), r))[:7]
        assert list(got7["order"][p, :len(want_rows)]) == want_rows
        assert got7["info"][p][0, 0] == len(want_rows)
    assert np.array_equal(got7["info"][1:3], got["info"][1:3]) and not np.array_equal(got7["info"][3:], got["info"][3:])
    other = truth_device(bank, c, 7, 6, ids)
    assert np.array_equal(other["hits"], got7["hits"]) and set(other["order"][4]) != set(got7["order"][4])


def test_seeded_scene_is_the_host_twin_bit_for_bit(seeded):
    sc, bank, c, got = seeded
    want = truth_host(bank.host(), c)
    same_bits(got, want, np.minimum(want["hits"][:, 1], want["order"].shape[1]))
    assert tuple(got["hits"][0]) == (3138, 3137) and tuple(got["hits"][4]) == (1, 0)


def test_seeded_scene_agrees_with_the_restatement(seeded):
    sc, bank, c, got = seeded
    assert go.check_pairs_against_restatement(bank.host(), c["frag1"], c["frag2"], c["Rt"], got, got["info"]) == 0


def test_two_calls_give_identical_bits(seeded):
    sc, bank, c, got = seeded
    again = truth_device(bank, c)
    same_bits(again, got, np.minimum(got["hits"][:, 1], got["order"].shape[1]))


@pytest.mark.parametrize("leaf", [None, 0.01])
def test_scene_ground_truth_equals_its_host_twin_for_every_batch_split(leaf):
    sc = go.seeded_scene()
    want_gt, want_info, want = gtm.scene_ground_truth_cpu(sc["clouds"], sc["poses"], leaf=leaf, num_threads=16)
    assert len(want_gt) == 12 if leaf is None else len(want_gt) > 0
    for batch in (1, 4, None):
        gt, gt_info, pp = gtm.scene_ground_truth(sc["clouds"], sc["poses"], DEV, leaf=leaf, batch_pairs=batch)
        assert [tuple(g.info) for g in gt] == [tuple(g.info) for g in want_gt] == [tuple(g.info) for g in gt_info]
        for g, w in zip(gt, want_gt):
            assert np.array_equal(g.trans, w.trans)
        for g, w in zip(gt_info, want_info):
            assert np.array_equal(g.mat.view(np.uint8), w.mat.view(np.uint8))
        for k in ("frag1", "frag2", "trans", "ratio", "hits", "info", "kept"):
            assert np.array_equal(pp[k], want[k]), (batch, k)


def test_nothing_synchronises_inside_the_pair_loop(seeded):
    sc, bank, c, got = seeded
    f1, f2, Rt = dev(c["frag1"]), dev(c["frag2"]), dev(c["Rt"])
    ids = torch.arange(len(c["frag1"]), dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:                                                               # raises if anything synchronises
        o = gtm.reach(bank, f1, f2, Rt, pair_ids=ids)
        info = gtm.correspondence_information(bank, f1, f2, Rt, o["key"], o["hits"])
        batched = gtm.pairs_ground_truth(bank, f1, f2, Rt, batch_pairs=4)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert np.array_equal(cpu(info), got["info"]) and np.array_equal(cpu(o["hits"]), got["hits"])
    for k in ("ratio", "hits", "info"):
        assert np.array_equal(cpu(batched[k]), got[k]), k


def test_scene_repeatability_on_the_device_is_its_host_twin():
    sc = go.seeded_scene()
    gt, _, _ = gtm.scene_ground_truth_cpu(sc["clouds"], sc["poses"], leaf=None, num_threads=16)
    M = max(len(x) for x in sc["xyz"])
    kp, count = np.zeros((6, 3, M), np.float32), np.array([len(x) for x in sc["xyz"]], np.int32)
    for f, x in enumerate(sc["xyz"]):
        kp[f, :, :len(x)] = x.T
    kp = kp + np.random.default_rng(3).normal(scale=0.03, size=kp.shape).astype(np.float32)
    want_ratio, want_hits = gtm.scene_repeatability_cpu(kp, count, gt, 0.05)
    ratio, hits = gtm.scene_repeatability(dev(kp), dev(count), gt, 0.05)
    assert np.array_equal(cpu(hits), want_hits) and np.array_equal(cpu(ratio), want_ratio) and 0 < want_hits.sum()
