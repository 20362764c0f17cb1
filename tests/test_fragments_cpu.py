"""Host twins of the f-9 fragment-registration entries (csrc/fragments_cpu.cpp over csrc/fragments_math.h) against the numpy
float64 restatement of the reference's MATLAB (tests/fragments_oracle.py, tests/eval_oracle.py).  The device runs the same
header; tests/test_fragments_gpu.py holds it to these twins.

The RANSAC bars are f-6's (tests/test_registration_cpu.py, derived there): 1e-9 on R, 1e-7 m on t, a trial left out when the
oracle's eigen-gap is below 1e-5 lambda_max or an oracle residual lies within 1e-7 m of the threshold, at most 1 % left out
-- and the fixtures here leave out none, which is asserted."""
import os
import sys

import numpy as np
import pytest

import eval_oracle as eo
import fragments_oracle as fo
from conftest import GOLDEN
from usip_amd import evaluation as ev
from usip_amd import fragments as fr

sys.path.insert(0, GOLDEN)
import make_tile_walk_golden as tw  # noqa: E402   (the cases of tests/golden/tile_walk_parent_bits.npz and how they are stored)

TOL_R, TOL_T = 1e-9, 1e-7
GAP, NEAR = 1e-5, 1e-7
THR = 0.2


# ------------------------------------------------------------------------------------------------ top-k matching
def check_topk(idx, valid, anc, pos, na, nb, k, what="host twin"):
    rows = unclear = wrong = 0
    for p in range(len(na)):
        want, clear = fo.topk(anc[p][:, :na[p]], pos[p][:, :nb[p]], k)
        kk = min(k, int(nb[p]))
        assert valid[p] == kk
        rows += int(na[p])
        unclear += int((~clear).sum())
        wrong += int((idx[p, :na[p], :kk] != want).any(1)[clear].sum())
        assert (idx[p, na[p]:] == 0).all() and (idx[p, :, kk:] == 0).all()
    print("%s k = %d: %d rows, %d unclear, %d mismatches elsewhere" % (what, k, rows, unclear, wrong))
    assert unclear <= 0.01 * rows and wrong == 0
    return unclear


@pytest.mark.parametrize("k", [1, 5, 8])
def test_topk_matching_against_oracle(k):
    anc, pos, na, nb = fo.topk_fixture()
    a2, p2 = anc.copy(), pos.copy()
    for p in range(len(na)):                                            # rows beyond the counts are never read
        a2[p, :, na[p]:] = np.nan
        p2[p, :, nb[p]:] = np.nan
    idx, valid = fr.match_descriptors_topk_cpu(a2, p2, na, nb, k)
    assert check_topk(idx, valid, anc, pos, na, nb, k) == 0             # the fixture leaves out no row
    i2, v2 = fr.match_descriptors_topk_cpu(a2, p2, na, nb, k, num_threads=5)
    assert np.array_equal(i2, idx) and np.array_equal(v2, valid)


@pytest.mark.parametrize("k", [2, 3, 4, 6, 7])
def test_topk_matching_against_oracle_at_the_remaining_k(k):
    """knn_counted_kernel<K> is instantiated for K = 1 .. 8: the five the test above leaves, on the same fixture."""
    test_topk_matching_against_oracle(k)


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 6, 7, 8])
def test_topk_awkward_shapes_against_oracle(k):
    """C = 33, Ma = 45 (a workgroup's four rows run past it), databases of 515, 257, 256 and 255 rows."""
    anc, pos, na, nb = fo.awkward_topk_fixture()
    a2, p2 = anc.copy(), pos.copy()
    for p in range(len(na)):                                            # rows beyond the counts are never read
        a2[p, :, na[p]:] = np.nan
        p2[p, :, nb[p]:] = np.nan
    idx, valid = fr.match_descriptors_topk_cpu(a2, p2, na, nb, k)
    assert check_topk(idx, valid, anc, pos, na, nb, k) == 0             # the fixture leaves out no row
    i2, v2 = fr.match_descriptors_topk_cpu(a2, p2, na, nb, k, num_threads=5)
    assert np.array_equal(i2, idx) and np.array_equal(v2, valid)
    if k == 1:
        assert np.array_equal(idx[:, :, 0], ev.match_descriptors_cpu(anc, pos, na, nb))


def tie_case():
    rng = np.random.default_rng(13)
    anc, pos = fo.unit_descriptors(rng, 1, 32, 40), fo.unit_descriptors(rng, 1, 32, 200)
    pos[0, :, 150] = pos[0, :, 20]                      # duplicates: the lower index first
    pos[0, :, 199] = pos[0, :, 70]
    pos[0, :, 71] = pos[0, :, 70]
    anc[0, :, 3] = pos[0, :, 20]
    anc[0, :, 4] = pos[0, :, 199]
    return anc, pos, np.array([40], np.int32), np.array([200], np.int32)


def test_topk_exact_ties_go_to_the_lower_index():
    anc, pos, na, nb = tie_case()
    idx, _ = fr.match_descriptors_topk_cpu(anc, pos, na, nb, 5)
    assert list(idx[0, 3, :2]) == [20, 150] and list(idx[0, 4, :3]) == [70, 71, 199]
    one, _ = fr.match_descriptors_topk_cpu(anc, pos, na, nb, 1)
    assert np.array_equal(one[0, :, 0], ev.match_descriptors_cpu(anc, pos, na, nb)[0])


def test_topk_at_k_1_is_the_one_nearest_entry_bit_for_bit():
    anc, pos, na, nb = fo.topk_fixture()
    idx, _, d = fr.match_descriptors_topk_cpu(anc, pos, na, nb, 1, want_dist=True)
    assert np.array_equal(idx[:, :, 0], ev.match_descriptors_cpu(anc, pos, na, nb))
    assert np.isinf(d[1]).all() and np.isfinite(d[0]).all()


# ------------------------------------------------------------------------------------------------ union
def union_cases():
    rng = np.random.default_rng(21)
    M, k = 64, 5
    nn12 = rng.integers(0, M, size=(1, M, k)).astype(np.int32)
    c = np.arange(k, dtype=np.int32) * 13
    spread = np.ascontiguousarray(((np.arange(M, dtype=np.int32)[:, None] + c) % M)[None])    # q = i + 13 c: every q k times
    back = np.ascontiguousarray(((np.arange(M, dtype=np.int32)[:, None] - c) % M)[None])      # i = q - 13 c: the same rows
    big = 1024
    return {"random": (nn12, rng.integers(0, M, size=(1, M, k)).astype(np.int32), [M], [M]),
            "full overlap": (spread, back, [M], [M]),
            "ragged": (nn12, rng.integers(0, 9, size=(1, M, k)).astype(np.int32), [9], [40]),
            "short lists": (nn12 % 3, rng.integers(0, M, size=(1, M, k)).astype(np.int32) % 50, [50], [3]),
            "empty": (nn12, nn12, [0], [0]),
            "Cmax at 10240": (rng.integers(0, big, size=(2, big, k)).astype(np.int32),
                              rng.integers(0, big, size=(2, big, k)).astype(np.int32), [big, big - 1], [big, 700])}


def check_union(pairs, count, nn12, nn21, n1, n2):
    k = nn12.shape[2]
    for p in range(len(n1)):
        k12, k21 = min(k, n2[p]), min(k, n1[p])
        want = fo.union(nn12[p, :n1[p], :k12], nn21[p, :n2[p], :k21])
        assert count[p] == len(want)
        assert np.array_equal(pairs[p, :count[p]], want) and (pairs[p, count[p]:] == 0).all()


@pytest.mark.parametrize("name", ["random", "full overlap", "ragged", "short lists", "empty", "Cmax at 10240"])
def test_union_equals_numpy_unique(name):
    nn12, nn21, n1, n2 = union_cases()[name]
    pairs, count = fr.match_union_cpu(nn12, nn21, np.asarray(n1, np.int32), np.asarray(n2, np.int32))
    check_union(pairs, count, nn12, nn21, n1, n2)
    if name == "full overlap":                                           # every row of the second list is in the first
        assert count[0] == 64 * 5


def test_union_disjoint_lists_keep_every_row():
    M, k = 64, 5
    c = np.arange(k, dtype=np.int32)
    nn12 = ((np.arange(M, dtype=np.int32)[:, None] + c) % M)[None]               # (i, q): q - i in 0 .. 4
    nn21 = ((np.arange(M, dtype=np.int32)[:, None] + 1 + c) % M)[None]           # (i, q): i - q in 1 .. 5
    full = np.array([M], np.int32)
    pairs, count = fr.match_union_cpu(np.ascontiguousarray(nn12), np.ascontiguousarray(nn21), full, full)
    check_union(pairs, count, nn12, nn21, [M], [M])
    assert count[0] == 2 * M * k


def test_union_refuses_more_than_10240():
    with pytest.raises(RuntimeError):
        fr.match_union_cpu(np.zeros((1, 1025, 5), np.int32), np.zeros((1, 1024, 5), np.int32), np.array([1], np.int32),
                           np.array([1], np.int32))


# ------------------------------------------------------------------------------------------------ RANSAC beyond 1024
def oracle_trials(batch):
    x1, x2, count, gt, tri = batch
    P, T = tri.shape[:2]
    Rt, cnt, gap, near = np.zeros((P, T, 3, 4)), np.zeros((P, T), int), np.zeros((P, T)), np.zeros((P, T))
    for p in range(P):
        for t in range(T):
            Rt[p, t], cnt[p, t], gap[p, t], near[p, t] = eo.trial(x1[p], x2[p], tri[p, t], THR)
    return Rt, cnt, gap, near


def check_trials(counts, hyp, oracle, what):
    Rt, cnt, gap, near = oracle
    keep = (gap >= GAP) & (near >= NEAR)
    err_r = np.abs(hyp[..., :3] - Rt[..., :3]).max((2, 3))
    err_t = np.abs(hyp[..., 3] - Rt[..., 3]).max(2)
    print("%s: left out %d of %d (smallest gap ratio %.2e, nearest residual %.2e m), max |dR| %.3e, max |dt| %.3e m, "
          "count mismatches %d" % (what, (~keep).sum(), keep.size, gap.min(), near.min(), err_r[keep].max(),
                                   err_t[keep].max(), (counts != cnt)[keep].sum()))
    assert 1.0 - keep.mean() <= 0.01
    assert err_r[keep].max() <= TOL_R and err_t[keep].max() <= TOL_T
    assert np.array_equal(counts[keep], cnt[keep])
    assert np.isfinite(hyp).all()
    return int((~keep).sum())


RANSAC_CASES = {3000: (3000, 400, 31), 10240: (10240, 150, 32)}          # n: (n, explicit trials, seed)
_ORACLES = {}


def ransac_case(n):
    if n not in _ORACLES:
        batch = fo.ransac_fixture(*RANSAC_CASES[n])
        _ORACLES[n] = (batch, oracle_trials(batch))
    return _ORACLES[n]


@pytest.mark.parametrize("n", [3000, 10240])
def test_ransac_per_trial_parity_beyond_1024(n):
    (x1, x2, count, gt, tri), oracle = ransac_case(n)
    counts, hyp, drawn = fr.ransac_trials_large_cpu(x1, x2, count, tri.shape[1], THR, triplets=tri)
    assert np.array_equal(drawn, tri)
    assert check_trials(counts, hyp, oracle, "host twin n = %d" % n) == 0      # the fixture leaves out no trial
    c2, h2, _ = fr.ransac_trials_large_cpu(x1, x2, count, tri.shape[1], THR, triplets=tri, num_threads=5)
    assert np.array_equal(c2, counts) and np.array_equal(h2, hyp)


def check_against_ransacfit(r, x1, x2, count, tri, max_trials):
    for p in range(len(count)):
        c = int(count[p])
        o = eo.ransacfit(x1[p][:, :c], x2[p][:, :c], THR, max_trials, tri[p])
        assert bool(r.valid[p]) == o["valid"], p
        assert (int(r.chosen[p]), int(r.trialcount[p])) == (o["chosen"], o["trialcount"]), p
        if not o["valid"]:
            assert np.array_equal(r.Rt[p], np.eye(3, 4)) and r.inliers[p] == 0 and not r.inlier_mask[p].any()
            assert r.inlier_ratio[p] == 0
            continue
        assert np.array_equal(np.nonzero(r.inlier_mask[p])[0], o["inliers"]) and r.inliers[p] == len(o["inliers"])
        assert r.inlier_ratio[p] == len(o["inliers"]) / c
        assert np.abs(r.Rt[p][:, :3] - o["Rt"][:, :3]).max() <= TOL_R and np.abs(r.Rt[p][:, 3] - o["Rt"][:, 3]).max() <= TOL_T


@pytest.mark.parametrize("n", [3000, 10240])
def test_ransac_end_to_end_beyond_1024(n):
    (x1, x2, count, gt, tri), _ = ransac_case(n)
    T = tri.shape[1]
    r = fr.fragment_registration_cpu(x1, x2, count, THR, T - 1, triplets=tri)
    check_against_ransacfit(r, x1, x2, count, tri, T - 1)
    assert r.valid[0] == 1 and r.inliers[0] > 0.3 * n
    assert eo.compare_transform(gt[0], r.Rt[0])[0] < 0.05


def test_ransac_small_counts_in_a_wide_batch():
    x1, x2, count, gt, tri = eo.make_batch(33, P=4, n=4, T=40, nmax=1500, counts=[0, 2, 3, 4], noise=0.01, inlier_share=1.0)
    r = fr.fragment_registration_cpu(x1, x2, count, THR, 39, triplets=tri)
    check_against_ransacfit(r, x1, x2, count, tri, 39)
    assert list(r.valid) == [0, 0, 1, 1] and list(r.trialcount[:3]) == [0, 0, 0]


def test_ransac_up_to_1024_is_the_existing_entry_bit_for_bit():
    x1, x2, count, gt, tri = eo.make_batch(34, P=4, n=1024, T=8, counts=[1024, 2, 300, 513], noise=0.01)
    ids = np.array([7, 8, 1000, 3], np.int64)
    for kw in (dict(seed=5, pair_ids=ids), dict(triplets=np.ascontiguousarray(np.repeat(tri, 50, 1)))):
        a = ev.ransac_registration_cpu(x1, x2, count, THR, 399, **kw)
        b = fr.fragment_registration_cpu(x1, x2, count, THR, 399, **kw)
        for f in ("inliers", "inlier_mask", "trialcount", "valid", "chosen", "counts"):
            assert np.array_equal(getattr(a, f), getattr(b, f)), f
        ok = a.valid != 0
        assert not ok[1] and ok.sum() >= 2
        assert np.array_equal(a.Rt[ok], b.Rt[ok]) and np.array_equal(b.Rt[~ok], np.broadcast_to(np.eye(3, 4), ((~ok).sum(), 3, 4)))


def test_large_entries_refuse_more_than_10240_and_the_existing_ones_keep_their_limit():
    x = np.zeros((1, 3, 10241), np.float32)
    with pytest.raises(RuntimeError):
        fr.ransac_trials_large_cpu(x, x, np.array([5], np.int32), 4)
    with pytest.raises(RuntimeError):
        ev.ransac_trials_cpu(x[:, :, :1025], x[:, :, :1025], np.array([5], np.int32), 4)


# ------------------------------------------------------------------------------------------------ information matrix
def test_information_matrix_within_the_summation_bound():
    rng = np.random.default_rng(41)
    P, N = 3, 3000
    x = rng.uniform(-4, 4, size=(P, 3, N)).astype(np.float32)
    mask = (rng.uniform(size=(P, N)) < 0.3).astype(np.uint8)
    mask[2] = 0
    info = fr.information_matrix_cpu(x, mask)
    for p in range(P):
        pts = x[p].T[mask[p] != 0]
        want, mag = fo.information(pts)
        n = len(pts)
        bound = 2 * n * 2.0 ** -53 * mag
        print("pair %d: %d points, max |twin - oracle| / bound %.3f" % (p, n, (np.abs(info[p] - want) / np.maximum(bound, 1e-300)).max()))
        assert (np.abs(info[p] - want) <= bound).all()
        assert np.array_equal(info[p], info[p].T)
        assert info[p][0, 0] == n
    assert not info[2].any()


# ------------------------------------------------------------------------------------------------ overlap
def test_overlap_hits_equal_brute_force():
    a, b, Rt = fo.room_pair(51)
    empty = np.zeros((0, 3), np.float32)
    bank = fr.host_bank([a, b, empty, a[:7]])
    f1, f2 = np.array([0, 1, 0, 2, 3], np.int32), np.array([1, 0, 2, 1, 1], np.int32)
    inv = np.concatenate((Rt[:, :3].T, -(Rt[:, :3].T @ Rt[:, 3:4])), 1)
    G = np.stack([Rt, inv, Rt, Rt, Rt])
    ratio, hits = fr.overlap_ratio_cpu(bank, f1, f2, G, 0.2)
    clouds = [a, b, empty, a[:7]]
    near_total = 0
    for p in range(len(f1)):
        h, r, near = fo.overlap(clouds[f1[p]], clouds[f2[p]], G[p], 0.2)
        near_total += near
        print("pair %d: hits %s oracle %s (near the radius: %d)" % (p, hits[p], h, near))
        assert np.array_equal(hits[p], h) and np.array_equal(ratio[p], r)
    assert near_total == 0                                               # the fixture has no point within 1e-9 of 0.2
    assert 0.3 < ratio[0, 0] < 0.7 and 0.3 < ratio[0, 1] < 0.7
    r2, h2 = fr.overlap_ratio_cpu(bank, f1, f2, G, 0.2, prune=False)     # the twin's own all-pairs answer
    assert np.array_equal(h2, hits) and np.array_equal(r2, ratio)
    r3, h3 = fr.overlap_ratio_cpu(bank, f1, f2, G, 0.2, num_threads=5)
    assert np.array_equal(h3, hits) and np.array_equal(r3, ratio)


def lattice_bank(size):
    """The lattice pair both ways round: (clouds, f1, f2, G, expected hits [P, 2]).  Pair 1 swaps the fragments and takes
    the inverse pose, so either direction's queries meet the equality cases as the moved side and as the static side."""
    a, b, Rt, hits, _ = fo.lattice_pair(size)
    f1, f2 = np.array([0, 1], np.int32), np.array([1, 0], np.int32)
    return [a, b], f1, f2, np.stack([Rt, fo.inverse_pose(Rt)]), np.stack([hits, hits[::-1]])


@pytest.mark.parametrize("threads", [1, 5])
@pytest.mark.parametrize("prune", [True, False])
@pytest.mark.parametrize("size", ["small", "large"])
def test_overlap_on_the_exact_lattice_equals_integer_arithmetic(size, prune, threads):
    """Hundreds of queries have their nearest point at exactly the radius (the fixture asserts it): sqrt(d2) < radius must
    say no to each of them, and yes to the planted partners at squared distance 398 and 393 of 400."""
    clouds, f1, f2, G, want = lattice_bank(size)
    ratio, hits = fr.overlap_ratio_cpu(fr.host_bank(clouds), f1, f2, G, fo.LATTICE_RADIUS, prune=prune, num_threads=threads)
    print("lattice %s: hits %s, integer oracle %s" % (size, hits.tolist(), want.tolist()))
    assert np.array_equal(hits, want)
    assert np.array_equal(ratio, want / np.array([[len(clouds[0]), len(clouds[1])], [len(clouds[1]), len(clouds[0])]]))


def wall_bank():
    """(clouds, f1, f2, G): the two rooms both ways round beside a 300-point, a 512-point and an empty fragment, so that
    Lmax padding and ragged lengths are in one launch."""
    clouds, Rt, _ = fo.wall_rooms()
    f1, f2 = np.array([0, 1, 2, 0, 0, 3, 4, 1], np.int32), np.array([1, 0, 1, 2, 3, 1, 1, 4], np.int32)
    inv = fo.inverse_pose(Rt)
    return clouds, f1, f2, np.stack([Rt, inv, Rt, inv, Rt, Rt, Rt, inv])


_WALL_ORACLE = {}


def wall_oracle():
    if not _WALL_ORACLE:
        clouds, f1, f2, G = wall_bank()
        got = [fo.tree_overlap(clouds[f1[p]], clouds[f2[p]], G[p], fo.WALL_RADIUS) for p in range(len(f1))]
        _WALL_ORACLE.update(hits=np.stack([g[0] for g in got]), ratio=np.stack([g[1] for g in got]),
                            near=sum(g[2] for g in got))
    return _WALL_ORACLE


def test_overlap_across_constant_x_walls_equals_the_tree():
    """Runs of about 16 700 equal x (65 tiles of the device's walk) in the static and in the moved fragment, at the
    benchmark's 100 000 points."""
    clouds, f1, f2, G = wall_bank()
    o = wall_oracle()
    ratio, hits = fr.overlap_ratio_cpu(fr.host_bank(clouds), f1, f2, G, fo.WALL_RADIUS, num_threads=16)
    print("walls: hits %s, tree %s (near the radius: %d)" % (hits.tolist(), o["hits"].tolist(), o["near"]))
    assert o["near"] == 0
    assert np.array_equal(hits, o["hits"]) and np.array_equal(ratio, o["ratio"])
    assert np.array_equal(hits[0], fo.wall_rooms()[2]) and np.array_equal(hits[1], hits[0][::-1])
    assert not hits[4].any() and not hits[5].any() and hits[2, 0] > 0 and hits[3, 1] > 0
    r2, h2 = fr.overlap_ratio_cpu(fr.host_bank(clouds), f1, f2, G, fo.WALL_RADIUS, prune=False, num_threads=16)
    assert np.array_equal(h2, hits) and np.array_equal(r2, ratio)


# ------------------------------------------------------------------------------------------------ the real configuration
_FULL = {}


def full_scene():
    """The scene of fragments_oracle.FULL_SCENE through the host twins at the reference's protocol (top 1024, k = 5,
    30 000 trials): (scene, stacked arrays, per-pair results), computed once for the CPU and the GPU tests."""
    if not _FULL:
        sc = fr.synthetic_scene(fo.FULL_SCENE["seed"], fo.FULL_SCENE["fragments"], fo.FULL_SCENE["points"],
                                landmarks=fo.FULL_SCENE["landmarks"])
        kp, de, cnt, f1, f2 = fo.stack_scene(sc, 1024)
        o = fr.register_pairs_cpu(kp[f1], de[f1], cnt[f1], kp[f2], de[f2], cnt[f2], fr.host_bank(sc["clouds"]), f1, f2,
                                  np.arange(len(f1)), num_threads=16)
        _FULL.update(sc=sc, stacked=(kp, de, cnt, f1, f2), per_pair=o)
    return _FULL["sc"], _FULL["stacked"], _FULL["per_pair"]


def test_full_size_scene_through_the_host_twins():
    """1024 keypoints, k = 5, 30 000 trials: the union is beyond 6000 rows (seven LDS chunks of the large kernels)."""
    sc, (kp, de, cnt, f1, f2), o = full_scene()
    assert tuple(cnt) == fo.FULL_KEYPOINTS and len(sc["gt"]) == 3
    assert tuple(o["matches"]) == fo.FULL_MATCHES and tuple(o["trialcount"]) == fo.FULL_TRIALCOUNT
    assert o["gate"].all() and o["valid"].all()
    s = fr.summarize(o, [0, 1, 2], sc["gt"], sc["gt_info"])
    assert {k: s[k] for k in fo.FULL_SCORE} == fo.FULL_SCORE
    over = fr.synthetic_scene(fo.FULL_SCENE["seed"], fo.FULL_SCENE["fragments"], fo.FULL_SCENE["points"], landmarks=1430,
                              ground_truth=False)
    assert max(len(x) for x in over["xyz"]) > 1024                       # what FragmentEvaluator(top=1024) refuses


# ------------------------------------------------------------------------------------------------ the score
def rot_z(a):
    return np.array([[np.cos(a), -np.sin(a), 0, 0], [np.sin(a), np.cos(a), 0, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]])


def test_transformation_error_against_the_restated_matlab():
    rng = np.random.default_rng(61)
    info = fo.information(rng.uniform(-3, 3, size=(50, 3)))[0]
    for _ in range(20):
        g = np.eye(4)
        g[:3, :3], g[:3, 3] = eo.random_rotation(rng, rng.uniform(0, 2)), rng.normal(size=3)
        r = g @ rot_z(rng.uniform(-0.2, 0.2))
        r[:3, 3] += rng.normal(0, 0.05, 3)
        assert abs(fr.transformation_error(g, r, info) - fo.transformation_error(g, r, info)) <= 1e-12
    assert fr.transformation_error(g, g, info) <= 1e-20
    flip = np.diag([-1.0, -1.0, 1.0, 1.0])                               # half a turn: trace -1, dcm2quat gives 0 / 0
    p = fr.transformation_error(np.eye(4), flip, info)
    assert np.isnan(p) and not p <= 0.04


def test_evaluate_log_on_hand_made_logs():
    n = 6
    info = np.diag([100.0, 100, 100, 400, 400, 400])
    gt = [fr.LogEntry((0, 1, n), np.eye(4)), fr.LogEntry((0, 2, n), rot_z(0.3)), fr.LogEntry((1, 3, n), np.eye(4)),
          fr.LogEntry((2, 5, n), np.eye(4)), fr.LogEntry((3, 5, n), np.eye(4))]
    gt_info = [fr.InfoEntry(g.info, info) for g in gt]
    at_bound = np.eye(4)
    at_bound[0, 3] = 0.2                                                 # p = 0.2^2 * 100 / 100 = 0.04 exactly: good
    over = np.eye(4)
    over[0, 3] = np.nextafter(0.2, 1.0) + 1e-9
    half_turn = np.diag([-1.0, -1.0, 1.0, 1.0])                          # trace -1 against gt = I: dcm2quat gives 0 / 0
    result = [fr.ResultEntry((0, 1, n), rot_z(2.0), 10, 0.5, info),      # consecutive: ignored, wrong as it is
              fr.ResultEntry((0, 2, n), rot_z(0.3), 40, 0.10, info),     # good
              fr.ResultEntry((1, 3, n), at_bound, 20, 0.05, info),       # good, at the bound
              fr.ResultEntry((2, 5, n), over, 99, 0.9, info),            # bad, just beyond it
              fr.ResultEntry((3, 5, n), half_turn, 99, 0.9, info),       # NaN: not good
              fr.ResultEntry((0, 4, n), np.eye(4), 99, 0.9, info)]       # not in gt: a false positive
    assert fr.transformation_error(np.eye(4), at_bound, info) == 0.04
    s = fr.evaluate_log(result, gt, gt_info)
    assert (s["gt_num"], s["rs_num"], s["good"], s["bad"], s["false_pos"]) == (4, 5, 2, 2, 1)
    assert s["recall"] == 2 / 4 and s["precision"] == 2 / 5
    assert s["inlier_num_mean"] == 30.0 and abs(s["inlier_ratio_mean"] - 0.075) <= 1e-15
    e = fr.evaluate_log([], gt, gt_info)
    assert e["recall"] == 0.0 and np.isnan(e["precision"]) and np.isnan(e["inlier_num_mean"]) and e["rs_num"] == 0
    assert fr.evaluate_log(result, gt, gt_info, err2=0.01)["good"] == 1


def test_gt_info_is_parsed_from_a_real_file():
    blocks = fr.read_info(os.path.join(GOLDEN, "redwood_gt_info_head.info"))
    assert [b.info for b in blocks] == [(0, 1, 57), (1, 2, 57), (3, 4, 57)]
    assert blocks[0].mat[0][0] == 3305 and blocks[0].mat.shape == (6, 6)
    assert blocks[0].mat[0][4] == 10048.00680351 and blocks[0].mat[4][0] == 10048.00680351
    assert blocks[2].mat[5][5] == 120139.75585331


def test_file_round_trips(tmp_path):
    rng = np.random.default_rng(71)
    sym = [fo.information(rng.uniform(-3, 3, size=(9, 3)))[0] for _ in range(3)]
    trans = [np.concatenate((np.concatenate((eo.random_rotation(rng, 1.0), rng.normal(size=(3, 1))), 1), [[0, 0, 0, 1.0]]))
             for _ in range(3)]
    heads = [(0, 2, 57), (3, 17, 57), (55, 56, 57)]
    log = [fr.LogEntry(h, t) for h, t in zip(heads, trans)]
    fr.write_log(str(tmp_path / "gt.log"), log)
    back = fr.read_log(str(tmp_path / "gt.log"))
    assert [b.info for b in back] == heads and all(np.abs(b.trans - t).max() <= 1e-8 for b, t in zip(back, trans))
    fr.write_info(str(tmp_path / "gt.info"), [fr.InfoEntry(h, m) for h, m in zip(heads, sym)])
    back = fr.read_info(str(tmp_path / "gt.info"))
    assert [b.info for b in back] == heads and all(np.abs(b.mat - m).max() <= 1e-8 for b, m in zip(back, sym))
    res = [fr.ResultEntry(h, t, 12 + i, 0.031 * (i + 1), m) for i, (h, t, m) in enumerate(zip(heads, trans, sym))]
    fr.write_result_log(str(tmp_path / "scene.log"), res)
    text = open(str(tmp_path / "scene.log")).read().split("\n")
    assert text[0] == "0\t 2\t 57\t" and text[5] == "12\t0.031000" and len(text[1].split("\t")) == 4   # writeLog.m's lines
    back = fr.read_result_log(str(tmp_path / "scene.log"))
    for b, r in zip(back, res):
        assert b.info == r.info and b.inlier_num == r.inlier_num and abs(b.inlier_ratio - r.inlier_ratio) <= 1e-6
        assert np.abs(b.trans - r.trans).max() <= 1e-10 and np.abs(b.information - r.information).max() <= 1e-10
    pf = fr.PairFile(3, 17, 41, 0.0625, (0.5, 0.25), trans[1], sym[1])
    fr.write_pair_file(str(tmp_path / "3-17.rt.txt"), pf)
    lines = open(str(tmp_path / "3-17.rt.txt")).read().split("\n")
    assert lines[0] == "3\t 17\t" and lines[1].startswith("41\t  6.25000000e-02\t") and len(lines) == 13
    b = fr.read_pair_file(str(tmp_path / "3-17.rt.txt"))
    assert (b.fragment1, b.fragment2, b.inlier_num, b.inlier_ratio, b.ratio_aligned) == (3, 17, 41, 0.0625, (0.5, 0.25))
    assert np.abs(b.trans - trans[1]).max() <= 1e-8 and np.abs(b.information - sym[1]).max() <= 1e-6 * np.abs(sym[1]).max()


def test_synthetic_scene_scores_one_through_the_host_twins():
    sc = fr.synthetic_scene(0, 6, 4000)
    F, top = 6, 128
    kp, de, cnt = np.zeros((F, 3, top), np.float32), np.zeros((F, 128, top), np.float32), np.zeros(F, np.int32)
    for i in range(F):
        n = len(sc["xyz"][i])
        kp[i, :, :n], de[i, :, :n], cnt[i] = sc["xyz"][i].T, sc["desc"][i].T, n
    pairs = [(i, j) for i in range(F) for j in range(i + 1, F)]
    f1, f2 = np.array([p[0] for p in pairs], np.int32), np.array([p[1] for p in pairs], np.int32)
    o = fr.register_pairs_cpu(kp[f1], de[f1], cnt[f1], kp[f2], de[f2], cnt[f2], fr.host_bank(sc["clouds"]), f1, f2,
                              np.arange(len(pairs)), num_threads=8)
    s = fr.summarize(o, list(range(F)), sc["gt"], sc["gt_info"])
    assert s["gt_num"] >= 6 and s["recall"] == 1.0 and s["precision"] == 1.0


# ------------------------------------------------------------------------------------------------ the pinned bits
@pytest.mark.parametrize("name", tw.OVERLAP)
def test_overlap_gives_the_bits_pinned_before_the_tile_walk_was_shared(name):
    """tests/golden/tile_walk_parent_bits.npz: (ratio, hits) of the twin before csrc/bank.h and csrc/host_split.h."""
    tw.check("overlap-" + name, tw.overlap_host(name), "host twin")


@pytest.mark.parametrize("registrator", tw.REGISTRATORS)
def test_register_pairs_cpu_gives_the_bits_pinned_before_it_ran_over_a_backend(registrator):
    """Every key of register_pairs_cpu with refine and dense_radius set, as the two copies of the pipeline returned them."""
    tw.check("pairs-" + registrator, tw.pairs_host(registrator), "host twins")
