"""CPU tests of tests/selection_oracle.py: what entitles the GPU tests of the selection kernels
(test_selection_kernels_gpu.py) to use it as the checker.  The float32 assignment and the exact cluster mean reproduce the
fixture the reference project recorded (tests/golden/som_cases.npz); every builder's claim -- tied rounds, pairs exactly at
the radius, the duplicate tail -- holds at the seeds the GPU tests use; the lattice references give the same answer twice."""
import numpy as np
import pytest
import torch

import selection_oracle as so
from conftest import assert_close, load_golden
from oracle import detector as od
from oracle import postproc


def test_lattice_draws_distinct_sites_while_they_last_and_is_exact():
    rng = np.random.default_rng(0)
    p = so.lattice(343, 7, rng)
    assert p.shape == (3, 343) and p.dtype == np.float32 and len(np.unique(p.T, axis=0)) == 343
    assert not np.array_equal(p, np.sort(p, axis=1))                       # shuffled
    q = so.lattice(500, 7, rng, 0.5)
    assert len(np.unique(q.T, axis=0)) < 500 and np.array_equal(q * 2, np.rint(q * 2)) and q.max() == 3.0
    d2 = ((p[:, :, None].astype(np.float64) - p[:, None, :]) ** 2).sum(axis=0)
    assert np.array_equal(d2, np.rint(d2)) and (d2 == 25).any() and (d2 == 1).any() and (d2 == 9).any()


def test_assignment_helper_reproduces_the_reference_projects_fixture():
    g = load_golden("som_cases.npz")
    min_idx, _ = so.som_assign_f32(g["x"], g["node"])
    assert np.array_equal(min_idx, g["min_idx"])
    M = g["node"].shape[2]
    mean, count, bound = so.som_cluster_exact(g["x"], min_idx, M)
    assert np.array_equal(count, g["count"])
    want_mean, _, want_dec = od.som_cluster(torch.from_numpy(g["x"]), torch.from_numpy(g["min_idx"]).long(),
                                            torch.from_numpy(g["count"]).long())
    assert_close(mean, want_mean.numpy(), name="cluster_mean")
    assert_close(so.som_decenter_f32(g["x"], mean, min_idx), want_dec.numpy(), name="x_decentered")
    assert (bound > 0).all() and (bound <= 2.0 * np.spacing(np.abs(mean)).astype(np.float64) + 1e-30).all()


def test_exact_mean_is_independent_of_the_order_and_sees_cancellation():
    """fsum of 1e8, 1, -1e8 is 1 (a float32 or a naive float64 running sum loses it to nothing or keeps it by luck); the
    bound of that node is far above ulp32(mean) only through sum|x|."""
    x = np.zeros((1, 3, 4), np.float32)
    x[0, 0] = [1e8, 1.0, -1e8, 0.5]
    idx = np.asarray([[0, 0, 0, 1]], np.int32)
    mean, count, bound = so.som_cluster_exact(x, idx, 3)
    assert count.tolist() == [[3, 1, 0]]
    assert mean[0, 0, 0] == np.float32(1.0) / (np.float32(3) + np.float32(1e-5))
    assert mean[0, 0, 1] == np.float32(0.5) / (np.float32(1) + np.float32(1e-5))
    assert mean[0, :, 2].tolist() == [0.0, 0.0, 0.0] and (bound[0, :, 2] == np.spacing(np.float32(0))).all()
    assert bound[0, 0, 0] > 3 * 2.0 ** -53 * 2e8 / 3.1
    with pytest.raises(AssertionError):
        so.som_cluster_exact(x, np.asarray([[0, 0, 0, 3]], np.int32), 3)


@pytest.mark.parametrize("name", sorted(so.FPS_CASES))
def test_fps_fixtures_hold_their_claims(name):
    """the floors the GPU test asserts, at its seeds; the reference gives the same answer twice"""
    args, floors = so.FPS_CASES[name]
    pts, first, want, claims = so.fps_lattice(*args)
    B, n, k = args[1], args[2], args[4]
    assert claims["tie"] >= floors[0] and claims["wave"] >= floors[1] and claims["slot"] >= floors[2], (claims, floors)
    assert n < B or len(set(first.tolist())) == B
    for b in range(B):
        again = postproc.fps_indices(pts[b].T, int(first[b]), k)
        assert np.array_equal(again, want[b]) and len(set(again.tolist())) == min(k, len(np.unique(pts[b].T, axis=0)))
    if name == "n16384_k64":
        assert int(want.max()) >= 15 * 1024                                # a pick out of the last slot
    if k == n:
        assert all(sorted(w.tolist()) == list(range(n)) for w in want)     # distinct points: a permutation


def test_fps_on_a_repeated_cloud_returns_index_zero_once_the_distinct_points_are_used_up():
    pts, first, want, claims = so.fps_repeated(17, 2, 40, 2000, 64)
    assert claims["used"] == 40 and claims["tie"] == 63 and claims["slot"] >= 40
    assert (first > 0).all() and not want[:, 40:].any() and (want[:, 1:40] > 0).any()
    for b in range(2):
        assert len(np.unique(pts[b].T, axis=0)) == 40


@pytest.mark.parametrize("name", sorted(so.NMS_CASES))
def test_nms_fixtures_hold_their_claims(name):
    args, floors = so.NMS_CASES[name]
    kp, sg = so.nms_lattice(*args[:4])
    assert len(np.unique(sg)) == 5 or sg.shape[1] == 1                     # sigmas drawn from five values
    order, count, claims = so.nms_reference(kp, sg, args[4])
    assert claims["at_radius"] >= floors[0] and claims["tie"] >= floors[1] and claims["wave"] >= floors[2], (claims, floors)
    order2, count2, claims2 = so.nms_reference(kp, sg, args[4])
    assert np.array_equal(order, order2) and np.array_equal(count, count2) and claims == claims2
    for b in range(args[1]):
        assert not order[b, count[b]:].any() and len(set(order[b, :count[b]].tolist())) == count[b]


def test_nms_one_ulp_below_the_radius_keeps_other_points():
    """r = 1 suppresses the lattice neighbours at distance exactly 1; the float32 just below 1 suppresses nobody on a
    lattice of distinct points: equality with the radius decides hundreds of keypoints"""
    args = so.NMS_CASES["m1024_r1"][0]
    kp, sg = so.nms_lattice(*args[:4])
    assert so.NMS_CASES["m1024_below_1"][0][:4] == args[:4] and so.BELOW_ONE < 1.0
    _, at_one, _ = so.nms_reference(kp, sg, 1.0)
    _, below, claims = so.nms_reference(kp, sg, so.BELOW_ONE)
    assert claims["at_radius"] == 0 and (below > at_one + 300).all() and (below == 1024).all()


def test_som_fixtures_hold_their_claims():
    for args, floor in so.SOM_CASES.values():
        x, node, want, claims = so.som_lattice(*args)
        assert claims["tied"] >= floor, (args, claims)
        assert want.min() >= 0 and want.max() < args[3]
    for M in (8, 9, 33):
        x, node, want, tied = so.som_hand_placed(M)
        got, got_tied = so.som_assign_f32(x, node)
        assert np.array_equal(got, want) and np.array_equal(got_tied, tied)
    for M in (8, 9):
        x, node, want, tied = so.som_hand_placed(M, duplicates=True)
        got, got_tied = so.som_assign_f32(x, node)
        assert np.array_equal(got, want) and np.array_equal(got_tied, tied)


def test_cluster_fixtures_hold_their_claims():
    for N, M in so.CLUSTER_SHAPES:
        x, idx, claims = so.cluster_case(N, M, "cancel")
        assert claims["cancel"] >= so.CANCEL_FLOOR, (N, M, claims)
        assert (np.abs(x) > 9e3).all() and (x > 0).any() and (x < 0).any() and idx.min() == 0 and idx.max() == M - 1
        assert so.cluster_case(N, M, "one_node")[2] == {"all": 1}
        if M > 1:
            assert so.cluster_case(N, M, "empty_node")[2] == {"empty": 0}


def test_knn_fixtures_tie_inside_and_across_the_kth_place():
    for N in sorted(so.KNN_SIDES):
        q, db, dist = so.knn_case(N)
        assert len(np.unique(db[0].T, axis=0)) == N                        # distinct database points
        for K in (1, 5, 64) + ((N,) if N <= 257 else ()):
            c, (inside, across) = so.knn_tie_claims(dist, K), so.knn_floors(N, K)
            assert c["rows"] == 140 and c["inside"] >= inside and c["across"] >= across, (N, K, c)
    q, db, dist = so.knn_case(257)
    idx, dist2 = so.knn_reference(q, db, 64)
    assert np.array_equal(dist, dist2)
    d = np.take_along_axis(dist, idx, axis=2)
    assert (d[:, :, 1:] >= d[:, :, :-1]).all()
    same = d[:, :, 1:] == d[:, :, :-1]
    assert (idx[:, :, 1:][same] > idx[:, :, :-1][same]).all()              # the lower index first on exact ties
    assert (d[:, :35, 0] == 0).all()                                       # the first half of the queries are database points
