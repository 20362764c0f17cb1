"""The f-9 fragment-registration kernels (csrc/fragments.hip) on the device against their host twins
(csrc/fragments_cpu.cpp, the same header in the same order) and against the numpy oracle (tests/fragments_oracle.py,
tests/eval_oracle.py).  Every output, discrete or float64, is compared with the twin's bit for bit: no tolerance is used
anywhere in this file except the oracle's own bars, which are those of tests/test_fragments_cpu.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import eval_oracle as eo
import fragments_oracle as fo
import test_fragments_cpu as tc
from conftest import ROOT
from usip_amd import evaluation as ev
from usip_amd import fragments as fr
from usip_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
THR = tc.THR


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


# ------------------------------------------------------------------------------------------------ top-k matching
@pytest.mark.parametrize("k", [1, 5, 8])
def test_topk_matching_equals_twin_and_oracle(k):
    anc, pos, na, nb = fo.topk_fixture()
    d, idx, valid = ops.knn_nd_counted(dev(anc), dev(pos), dev(na), dev(nb), k)
    ti, tv, td = fr.match_descriptors_topk_cpu(anc, pos, na, nb, k, want_dist=True)
    assert np.array_equal(host(idx), ti) and np.array_equal(host(valid), tv)
    assert np.array_equal(host(d).view(np.uint32), td.view(np.uint32))
    assert tc.check_topk(host(idx), host(valid), anc, pos, na, nb, k, "device") == 0


def test_topk_at_k_1_is_the_one_nearest_kernel_bit_for_bit():
    anc, pos, na, nb = fo.topk_fixture()
    d, idx, _ = ops.knn_nd_counted(dev(anc), dev(pos), dev(na), dev(nb), 1)
    d1, i1 = ops.nearest_nd_counted(dev(anc), dev(pos), dev(na), dev(nb))
    assert torch.equal(idx[:, :, 0], i1) and torch.equal(d[:, :, 0].view(torch.int32), d1.view(torch.int32))


def topk_device_case(fixture, k):
    """Device against twin (indices, valid, distance bits) and against the oracle; rows and columns beyond the counts
    are NaN: they are never read."""
    anc, pos, na, nb = fixture
    a2, p2 = anc.copy(), pos.copy()
    for p in range(len(na)):
        a2[p, :, na[p]:] = np.nan
        p2[p, :, nb[p]:] = np.nan
    d, idx, valid = ops.knn_nd_counted(dev(a2), dev(p2), dev(na), dev(nb), k)
    ti, tv, td = fr.match_descriptors_topk_cpu(a2, p2, na, nb, k, want_dist=True)
    assert np.array_equal(host(idx), ti) and np.array_equal(host(valid), tv)
    assert np.array_equal(host(d).view(np.uint32), td.view(np.uint32))
    assert tc.check_topk(host(idx), host(valid), anc, pos, na, nb, k, "device") == 0
    return a2, p2, d, idx


@pytest.mark.parametrize("k", [2, 3, 4, 6, 7])
def test_topk_matching_equals_twin_and_oracle_at_the_remaining_k(k):
    """knn_counted_kernel<K> is instantiated for K = 1 .. 8; the test above runs three of them."""
    topk_device_case(fo.topk_fixture(), k)


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 6, 7, 8])
def test_topk_awkward_shapes_equal_twin_and_oracle(k):
    """C = 33; Ma = 45, so the last workgroup's rows 45 .. 47 leave at `i >= Ma`; databases of 515, 257, 256 and 255 rows
    around one pass of a wave (64 * NJ = 256), where the tail clamp min(j, nb - 1) decides what is read."""
    a2, p2, d, idx = topk_device_case(fo.awkward_topk_fixture(), k)
    if k == 1:
        _, _, na, nb = fo.awkward_topk_fixture()
        d1, i1 = ops.nearest_nd_counted(dev(a2), dev(p2), dev(na), dev(nb))
        assert torch.equal(idx[:, :, 0], i1) and torch.equal(d[:, :, 0].view(torch.int32), d1.view(torch.int32))


def test_topk_ties_and_wide_batches():
    anc, pos, na, nb = tc.tie_case()
    idx, _ = fr.match_descriptors_topk(dev(anc), dev(pos), dev(na), dev(nb), 5)
    assert np.array_equal(host(idx), fr.match_descriptors_topk_cpu(anc, pos, na, nb, 5)[0])
    assert list(host(idx)[0, 3, :2]) == [20, 150] and list(host(idx)[0, 4, :3]) == [70, 71, 199]
    rng = np.random.default_rng(81)                                       # more candidates than one pass of a wave holds
    a, b = fo.unit_descriptors(rng, 3, 128, 512), fo.unit_descriptors(rng, 3, 128, 1024)
    b[1, :, 700] = b[1, :, 3]
    na, nb = np.array([512, 300, 511], np.int32), np.array([1024, 1023, 257], np.int32)
    for k in (5, 8):
        idx, valid = fr.match_descriptors_topk(dev(a), dev(b), dev(na), dev(nb), k)
        ti, tv = fr.match_descriptors_topk_cpu(a, b, na, nb, k, num_threads=8)
        assert np.array_equal(host(idx), ti) and np.array_equal(host(valid), tv)


# ------------------------------------------------------------------------------------------------ union
@pytest.mark.parametrize("name", ["random", "full overlap", "ragged", "short lists", "empty", "Cmax at 10240"])
def test_union_equals_twin_and_numpy_unique(name):
    nn12, nn21, n1, n2 = tc.union_cases()[name]
    c1, c2 = np.asarray(n1, np.int32), np.asarray(n2, np.int32)
    pairs, count = fr.match_union(dev(nn12), dev(nn21), dev(c1), dev(c2))
    tp, tn = fr.match_union_cpu(nn12, nn21, c1, c2)
    assert np.array_equal(host(pairs), tp) and np.array_equal(host(count), tn)
    tc.check_union(host(pairs), host(count), nn12, nn21, n1, n2)


def test_union_lengths_around_the_powers_of_two():
    rng = np.random.default_rng(82)
    for M in (51, 52, 102, 103, 205):                                    # totals 2 k M: 510, 520, 1020, 1030, 2050
        nn12 = rng.integers(0, M, size=(2, M, 5)).astype(np.int32)
        nn21 = rng.integers(0, M, size=(2, M, 5)).astype(np.int32)
        c = np.array([M, M - 1], np.int32)
        pairs, count = fr.match_union(dev(nn12), dev(nn21), dev(c), dev(c))
        tc.check_union(host(pairs), host(count), nn12, nn21, list(c), list(c))
    with pytest.raises(RuntimeError):
        fr.match_union(dev(np.zeros((1, 1025, 5), np.int32)), dev(np.zeros((1, 1024, 5), np.int32)),
                       dev(np.array([1], np.int32)), dev(np.array([1], np.int32)))


# ------------------------------------------------------------------------------------------------ RANSAC beyond 1024
def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


@pytest.mark.parametrize("n", [3000, 10240])
def test_ransac_trials_equal_twin_on_all_trials_and_hold_the_oracle_bars(n):
    """Hypotheses are held to the twin's bit for bit, as f-6 measured for its own kernels; the largest difference is
    printed before the assertion."""
    (x1, x2, count, gt, tri), oracle = tc.ransac_case(n)
    T = tri.shape[1]
    counts, hyp, _ = ops.ransac_trials_large(dev(x1), dev(x2), dev(count), T, THR, triplets=dev(tri), want_hypotheses=True)
    tcounts, thyp, _ = fr.ransac_trials_large_cpu(x1, x2, count, T, THR, triplets=tri, num_threads=8)
    assert np.array_equal(host(counts), tcounts)                         # ALL trials
    print("n = %d: max |device - twin| on hypotheses %.3e" % (n, np.abs(host(hyp) - thyp).max()))
    assert same_bits(host(hyp), thyp)
    assert tc.check_trials(host(counts), host(hyp), oracle, "device n = %d" % n) == 0
    r = fr.fragment_registration(dev(x1), dev(x2), dev(count), THR, T - 1, triplets=dev(tri))
    rh = fr.FragmentResult(*[host(f) if f is not None else None for f in r])
    tc.check_against_ransacfit(rh, x1, x2, count, tri, T - 1)
    t = fr.fragment_registration_cpu(x1, x2, count, THR, T - 1, triplets=tri)
    compare_results(rh, t)


def compare_results(a, b):
    for f in ("inliers", "inlier_mask", "trialcount", "valid", "chosen", "counts"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    assert same_bits(a.Rt, b.Rt) and same_bits(a.inlier_ratio, b.inlier_ratio)


def test_philox_draws_small_counts_and_chunk_edges():
    """Philox draws on ragged batches whose counts sit one below, at and one above a multiple of the 1024-row LDS chunk,
    and the counts 0, 2, 3, 4."""
    counts = [1023, 1024, 1025, 2047, 2048, 2049, 0, 2, 3, 4, 3071, 10240]
    x1, x2, count, gt, tri = eo.make_batch(91, P=len(counts), n=10240, T=1, counts=counts, noise=0.02)
    ids = np.arange(100, 100 + len(counts), dtype=np.int64)
    r = fr.fragment_registration(dev(x1), dev(x2), dev(count), THR, 600, 17, dev(ids))
    rh = fr.FragmentResult(*[host(f) if f is not None else None for f in r])
    t = fr.fragment_registration_cpu(x1, x2, count, THR, 600, 17, ids, num_threads=16)
    compare_results(rh, t)
    assert list(rh.valid[6:9]) == [0, 0, 1] and rh.trialcount[9] == 601 and rh.valid[[0, 1, 2, 3, 4, 5, 10, 11]].all()
    assert np.array_equal(rh.Rt[6], np.eye(3, 4)) and not rh.inlier_mask[6].any()
    _, _, drawn = ops.ransac_trials_large(dev(x1), dev(x2), dev(count), 50, THR, 17, dev(ids), want_triplets=True)
    assert np.array_equal(host(drawn), fr.ransac_trials_large_cpu(x1, x2, count, 50, THR, 17, ids)[2])


def test_up_to_1024_the_large_entries_are_the_existing_ones_bit_for_bit():
    x1, x2, count, gt, tri = eo.make_batch(34, P=4, n=1024, T=8, counts=[1024, 2, 300, 513], noise=0.01)
    ids = dev(np.array([7, 8, 1000, 3], np.int64))
    a = ev.ransac_registration(dev(x1), dev(x2), dev(count), THR, 1999, 5, ids)
    b = fr.fragment_registration(dev(x1), dev(x2), dev(count), THR, 1999, 5, ids)
    for f in ("inliers", "inlier_mask", "trialcount", "valid", "chosen", "counts"):
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    ok = a.valid != 0
    assert not bool(ok[1]) and int(ok.sum()) >= 2
    assert torch.equal(a.Rt[ok].view(torch.int64), b.Rt[ok].view(torch.int64))
    ca, ha, _ = ops.ransac_trials(dev(x1), dev(x2), dev(count), 700, THR, 5, ids, want_hypotheses=True)
    cb, hb, _ = ops.ransac_trials_large(dev(x1), dev(x2), dev(count), 700, THR, 5, ids, want_hypotheses=True)
    assert torch.equal(ca, cb) and torch.equal(ha.view(torch.int64), hb.view(torch.int64))
    with pytest.raises(RuntimeError):
        ops.ransac_trials(dev(np.zeros((1, 3, 1025), np.float32)), dev(np.zeros((1, 3, 1025), np.float32)),
                          dev(np.array([5], np.int32)), 4, THR)


def test_large_entries_take_a_count_outside_0_to_nmax_as_the_nearer_end():
    """clamp_count of the large kernels: a count above Nmax behaves as Nmax and a count below 0 as 0, draws included."""
    x1, x2, count, gt, tri = eo.make_batch(36, P=4, n=3000, T=1, noise=0.05)
    ids = np.array([40, 41, 42, 43], np.int64)
    wild, tame = np.array([5000, 3000, -7, 0], np.int32), np.array([3000, 3000, 0, 0], np.int32)
    got = {}
    for name, c in (("wild", wild), ("tame", tame)):
        r = fr.fragment_registration(dev(x1), dev(x2), dev(c), THR, 700, 23, dev(ids))
        got[name] = fr.FragmentResult(*[host(f) if f is not None else None for f in r])
        compare_results(got[name], fr.fragment_registration_cpu(x1, x2, c, THR, 700, 23, ids, num_threads=16))
    for f in ("inliers", "inlier_mask", "trialcount", "valid", "chosen", "counts"):
        assert np.array_equal(getattr(got["wild"], f), getattr(got["tame"], f)), f
    assert same_bits(got["wild"].Rt, got["tame"].Rt)
    w = got["wild"]
    assert list(w.valid) == [1, 1, 0, 0] and w.inliers[0] > 900 and not w.inlier_mask[2:].any() and not w.counts[2:].any()
    assert np.array_equal(w.Rt[2], np.eye(3, 4)) and list(w.trialcount[2:]) == [0, 0]
    _, _, drawn = ops.ransac_trials_large(dev(x1), dev(x2), dev(wild), 50, THR, 23, dev(ids), want_triplets=True)
    assert np.array_equal(host(drawn), fr.ransac_trials_large_cpu(x1, x2, tame, 50, THR, 23, ids)[2])
    assert host(drawn)[:2].max() >= 2900 and host(drawn).max() < 3000


@pytest.mark.parametrize("at", [254, 255, 256, 257, 511, 512])
def test_stopping_rule_exits_on_either_side_of_a_scan_edge(at):
    """The select kernel scans 256 trials at a time; the loop's exit is placed just before, at and after an edge."""
    n, b = 2000, 1200
    scores = [3] * at + [b] + [3] * 300                                   # the budget of b has passed when it arrives
    T = len(scores)
    assert eo.replay(scores, n, T - 1) == (at, at + 1)
    x1, x2, count, gt, tri = eo.make_batch(5, P=1, n=n, T=T, noise=0.02)
    counts = np.asarray(scores, np.int32)[None]
    o = ops.ransac_select_large(dev(x1), dev(x2), dev(count), dev(counts), T - 1, THR, triplets=dev(tri))
    t = fr.ransac_select_large_cpu(x1, x2, count, counts, T - 1, THR, triplets=tri)
    assert (int(o["chosen"][0]), int(o["trialcount"][0])) == (at, at + 1)
    for f in ("inliers", "inlier_mask", "trialcount", "valid", "chosen"):
        assert np.array_equal(host(o[f]), t[f]), f
    assert same_bits(host(o["Rt"]), t["Rt"])


# ------------------------------------------------------------------------------------------------ information, overlap
def test_information_matrix_equals_twin_and_holds_the_summation_bound():
    rng = np.random.default_rng(41)
    P, N = 4, 5000
    x = rng.uniform(-4, 4, size=(P, 3, N)).astype(np.float32)
    mask = (rng.uniform(size=(P, N)) < 0.3).astype(np.uint8)
    mask[2] = 0
    mask[3] = 1
    info = host(fr.information_matrix(dev(x), dev(mask)))
    assert same_bits(info, fr.information_matrix_cpu(x, mask))
    for p in range(P):
        pts = x[p].T[mask[p] != 0]
        want, mag = fo.information(pts)
        assert (np.abs(info[p] - want) <= 2 * len(pts) * 2.0 ** -53 * mag).all()
        assert np.array_equal(info[p], info[p].T) and info[p][0, 0] == len(pts)
    assert not info[2].any()


def test_overlap_equals_twin_and_brute_force():
    a, b, Rt = fo.room_pair(51)
    empty = np.zeros((0, 3), np.float32)
    clouds = [a, b, empty, a[:7], b[:300]]
    f1, f2 = np.array([0, 1, 0, 2, 3, 0, 4], np.int32), np.array([1, 0, 2, 1, 1, 4, 0], np.int32)
    inv = np.concatenate((Rt[:, :3].T, -(Rt[:, :3].T @ Rt[:, 3:4])), 1)
    G = np.stack([Rt, inv, Rt, Rt, Rt, Rt, inv])
    bank = fr.FragmentBank(clouds, DEV)
    ratio, hits = fr.overlap_ratio(bank, dev(f1), dev(f2), dev(G), 0.2)
    tr, th = fr.overlap_ratio_cpu(fr.host_bank(clouds), f1, f2, G, 0.2, num_threads=8)
    assert np.array_equal(host(hits), th) and same_bits(host(ratio), tr)
    near = 0
    for p in range(len(f1)):
        h, r, nr = fo.overlap(clouds[f1[p]], clouds[f2[p]], G[p], 0.2)
        near += nr
        assert np.array_equal(host(hits)[p], h) and np.array_equal(host(ratio)[p], r)
    assert near == 0 and 0.3 < float(ratio[0, 0]) < 0.7
    hb = bank.host()
    assert np.array_equal(hb.rows, fr.host_bank(clouds).rows) and np.array_equal(hb.offsets, fr.host_bank(clouds).offsets)


def device_overlap(clouds, f1, f2, G, radius):
    ratio, hits = fr.overlap_ratio(fr.FragmentBank(clouds, DEV), dev(f1), dev(f2), dev(G), radius)
    return host(ratio), host(hits)


@pytest.mark.parametrize("size", ["small", "large"])
def test_overlap_on_the_exact_lattice_equals_integer_arithmetic(size):
    """Pair 0 is the lattice under Rt, pair 1 the fragments swapped under the inverse: either instantiation of
    overlap_kernel<XQ> meets the queries whose nearest point is at exactly the radius from both sides."""
    clouds, f1, f2, G, want = tc.lattice_bank(size)
    ratio, hits = device_overlap(clouds, f1, f2, G, fo.LATTICE_RADIUS)
    print("lattice %s: device hits %s, integer oracle %s, decided by equality alone %s"
          % (size, hits.tolist(), want.tolist(), fo.lattice_pair(size)[4].tolist()))
    assert np.array_equal(hits, want)
    tr, th = fr.overlap_ratio_cpu(fr.host_bank(clouds), f1, f2, G, fo.LATTICE_RADIUS, num_threads=16)
    assert np.array_equal(hits, th) and same_bits(ratio, tr)
    assert np.array_equal(hits, fr.overlap_ratio_cpu(fr.host_bank(clouds), f1, f2, G, fo.LATTICE_RADIUS, prune=False,
                                                     num_threads=16)[1])


def test_overlap_across_constant_x_walls_equals_twin_and_tree():
    """100 000-point rooms (391 tiles) whose static and moved x hold runs of about 16 700 equal values (65 tiles), beside
    300-, 512- and 0-point fragments in the same launch."""
    clouds, f1, f2, G = tc.wall_bank()
    o = tc.wall_oracle()
    ratio, hits = device_overlap(clouds, f1, f2, G, fo.WALL_RADIUS)
    print("walls: device hits %s, tree %s" % (hits.tolist(), o["hits"].tolist()))
    assert o["near"] == 0 and np.array_equal(hits, o["hits"]) and np.array_equal(ratio, o["ratio"])
    tr, th = fr.overlap_ratio_cpu(fr.host_bank(clouds), f1, f2, G, fo.WALL_RADIUS, num_threads=16)
    assert np.array_equal(hits, th) and same_bits(ratio, tr)
    assert np.array_equal(hits, fr.overlap_ratio_cpu(fr.host_bank(clouds), f1, f2, G, fo.WALL_RADIUS, prune=False,
                                                     num_threads=16)[1])


def test_overlap_of_fragments_50_m_apart_is_exactly_zero():
    """Fragment 2 moved 50 m along x, once to either side: for one instantiation every binary search ends at lo == nd
    (with nd = 512 the start tile is the clamp's tiles - 1), for the other at 0, and no tile is within the radius."""
    clouds, Rt, _ = fo.wall_rooms()
    f1, f2 = np.array([0, 0, 0, 0, 2, 4], np.int32), np.array([1, 1, 4, 4, 1, 0], np.int32)
    up, down = fo.far_pose(Rt, 50.0), fo.far_pose(Rt, -50.0)
    G = np.stack([up, down, up, down, down, up])
    ratio, hits = device_overlap(clouds, f1, f2, G, fo.WALL_RADIUS)
    assert not hits.any() and not ratio.any()
    assert not fr.overlap_ratio_cpu(fr.host_bank(clouds), f1, f2, G, fo.WALL_RADIUS, num_threads=16)[1].any()


# ------------------------------------------------------------------------------------------------ the evaluator
def scene_evaluator(sc, **kw):
    e = fr.FragmentEvaluator(None, None, None, DEV, top=128, **kw)
    for i in range(len(sc["clouds"])):
        e.add_fragment_result(i, sc["xyz"][i], sc["desc"][i], sc["clouds"][i])
    return e


def test_evaluator_equals_the_pipeline_of_host_twins_without_synchronising():
    sc = fr.synthetic_scene(0, 6, 4000)
    e = scene_evaluator(sc, batch_pairs=4)
    bank = e.bank()                                                       # uploads and the static sort: before the pairs
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        per_pair = e.evaluate_device()                                    # raises if anything synchronises
    finally:
        torch.cuda.set_sync_debug_mode("default")
    got = {k: host(v) for k, v in per_pair.items()}
    s = fr.summarize(got, e.ids(), sc["gt"], sc["gt_info"])
    kp, de, cnt = [host(t) for t in e.stacked()]
    pairs = e.all_pairs()
    f1, f2 = np.array([p[0] for p in pairs], np.int32), np.array([p[1] for p in pairs], np.int32)
    want = []
    for base in range(0, len(pairs), 4):                                  # pair ids as the evaluator numbers them
        sl = slice(base, base + 4)
        want.append(fr.register_pairs_cpu(kp[f1[sl]], de[f1[sl]], cnt[f1[sl]], kp[f2[sl]], de[f2[sl]], cnt[f2[sl]],
                                          bank.host(), f1[sl], f2[sl], np.arange(base, base + len(f1[sl])), num_threads=16))
    want = {k: np.concatenate([w[k] for w in want]) for k in want[0]}
    assert set(got) == set(want)
    for k in want:
        if want[k].dtype == np.float64:
            assert same_bits(got[k], want[k]), k
        else:
            assert np.array_equal(got[k], want[k]), k
    t = fr.summarize(want, e.ids(), sc["gt"], sc["gt_info"])
    assert (s["recall"], s["precision"], s["good"], s["written"]) == (t["recall"], t["precision"], t["good"], t["written"])
    assert s["recall"] == 1.0 and s["precision"] == 1.0 and s["gt_num"] >= 6
    full = e.evaluate(None, sc["gt"], sc["gt_info"])                      # the public call: the same numbers
    assert full["recall"] == 1.0 and full["pairs"] == 15 and same_bits(full["per_pair"]["Rt"], got["Rt"])


def full_evaluator(sc, stage=lambda t: t):
    e = fr.FragmentEvaluator(None, None, None, DEV, top=1024)            # the reference's protocol: k = 5, 30 000 trials
    for i in range(len(sc["clouds"])):
        e.add_fragment_result(i, stage(dev(sc["xyz"][i])), stage(dev(sc["desc"][i])), stage(dev(sc["clouds"][i])))
    return e


def same_outputs(got, want):
    assert set(got) == set(want)
    for k in want:
        a, b = (host(v) if isinstance(v, torch.Tensor) else v for v in (got[k], want[k]))
        assert a.dtype == b.dtype, k
        if b.dtype == np.float64:
            assert same_bits(a, b), k
        else:
            assert np.array_equal(a, b), k


def test_evaluator_at_the_reference_protocol_equals_the_host_twins_without_synchronising():
    """1024 keypoints, k = 5, 30 000 trials: unions beyond 6000 rows, so the large kernels walk seven LDS chunks and the
    select kernel keeps its flags in the mask, chained as the benchmark chains them."""
    sc, _, want = tc.full_scene()
    e = full_evaluator(sc)
    e.bank()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        per_pair = e.evaluate_device()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    got = {k: host(v) for k, v in per_pair.items()}
    same_outputs(got, want)
    assert tuple(got["matches"]) == fo.FULL_MATCHES and tuple(got["trialcount"]) == fo.FULL_TRIALCOUNT
    s = fr.summarize(got, e.ids(), sc["gt"], sc["gt_info"])
    assert s["recall"] == 1.0 and s["precision"] == 1.0 and {k: s[k] for k in fo.FULL_SCORE} == fo.FULL_SCORE
    over = fr.synthetic_scene(fo.FULL_SCENE["seed"], fo.FULL_SCENE["fragments"], fo.FULL_SCENE["points"], landmarks=1430,
                              ground_truth=False)
    with pytest.raises(ValueError):                                      # more than 1024 keypoints in a fragment
        full_evaluator(over)


def test_two_calls_agree_and_a_side_stream_is_ordered():
    sc, _, want = tc.full_scene()
    e = full_evaluator(sc)
    first = e.evaluate_device()
    second = e.evaluate_device()
    same_outputs(first, want)
    same_outputs(second, want)
    # the fragments are produced on the side stream right before the call: only stream order makes the result right
    torch.cuda.synchronize()
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream())

    def ahead(t):
        for _ in range(50):                                              # work ahead of the call on the same stream;
            t = t * 1.0                                                  # (x * 1.0 is exact: the values are unchanged)
        return t
    with torch.cuda.stream(side):
        third = full_evaluator(sc, ahead).evaluate_device()
    side.synchronize()
    same_outputs(third, want)


def test_sync_debug_mode_sees_a_host_read():
    """The guard of the test above is not vacuous: a host read under it raises."""
    x = torch.ones(4, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            x.sum().item()
    finally:
        torch.cuda.set_sync_debug_mode("default")


def test_example_scores_recall_one_on_the_synthetic_scene(tmp_path):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "evaluate_fragments.py"), "--make-synthetic",
                          str(tmp_path / "scene"), "--fragments", "6", "--points", "4000"], capture_output=True, text=True,
                         timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    res = json.loads(lines[0])
    assert res["recall"] == 1.0 and res["precision"] == 1.0 and res["pairs"] == 15
    log = fr.read_result_log(str(tmp_path / "scene" / "results" / "synthetic.log"))
    assert len(log) == res["written"] and os.path.exists(str(tmp_path / "scene" / "results" / "synthetic" / "0.bin"))


@pytest.mark.parametrize("name", tc.tw.OVERLAP)
def test_overlap_on_the_device_gives_the_pinned_parent_bits(name):
    """tests/golden/tile_walk_parent_bits.npz through overlap_kernel<XQ> over csrc/tile_walk.h: a partial last tile, the
    binary search at lo == nd with the start tile clamped, constant-x runs of 65 tiles, an empty fragment."""
    tc.tw.check("overlap-" + name, tc.tw.overlap_device(name, DEV), "device")


@pytest.mark.parametrize("registrator", tc.tw.REGISTRATORS)
def test_register_pairs_on_the_device_gives_the_pinned_parent_bits(registrator):
    tc.tw.check("pairs-" + registrator, tc.tw.pairs_device(registrator, DEV), "device")
