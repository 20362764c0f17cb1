"""The selection kernels whose result is an index -- usip_fps_f32, usip_nms_f32 (csrc/fps.hip), usip_som_assign_f32,
usip_som_cluster(_csr)_f32 and the decentring (csrc/som.hip), usip_knn_f32 and usip_knn_points_f32 (csrc/knn.hip) -- on
the MI355X at exact ties and at their limits, against the plain references of tests/selection_oracle.py (which
test_selection_oracle_cpu.py anchors to the reference project's fixture).

Lattice inputs make every distance exact, so the "first maximum / first minimum / lower index" rules are defined without
any rounding and every index is compared BIT FOR BIT; each test first asserts that its fixture ties where it claims to
(selection_oracle's floors).  The one comparison that is not exact is the cluster mean, held to
ulp32(want) + c 2^-53 sum|x| / denom, the bound that follows from the kernels' stated arithmetic (double sums, one rounding
to float32, one float32 division); it prints its worst err / bound (run with -s to see them).  Measured on one MI355X,
scan and segment walk alike: normal 0.00, cancel 0.00, empty_node 0.00, one_node 0.00 -- every mean came out as the
reference's own bits.  No bound was widened after a run."""
import numpy as np
import pytest
import torch

import selection_oracle as so

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def _ops():
    from usip_amd import ops
    return ops


def _same_indices(got, want, what):
    got = host(got)
    assert got.dtype == np.int32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "%s: %d of %d differ, first at %s: got %d, want %d" % (
        what, len(bad), want.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


# =============================================================================================== usip_fps_f32
@pytest.mark.parametrize("name", sorted(so.FPS_CASES))
def test_fps_on_a_lattice_takes_the_first_maximum(name):
    """every round's maximum is shared by several points, in other lanes, other waves and other slots of their thread:
    the per-thread scan, the 64-lane butterfly and the 16-wave merge must all hand on the LOWEST index"""
    args, floors = so.FPS_CASES[name]
    pts, first, want, claims = so.fps_lattice(*args)
    assert claims["tie"] >= floors[0] and claims["wave"] >= floors[1] and claims["slot"] >= floors[2], (claims, floors)
    got = _ops().fps(dev(pts), dev(first), args[4])
    _same_indices(got, want, "fps " + name)
    if args[4] == args[2]:                                                 # k == n on distinct points: a permutation
        assert all(sorted(row.tolist()) == list(range(args[2])) for row in host(got))


def test_fps_on_a_cloud_padded_by_repetition_ends_in_index_zero():
    """40 distinct points repeated to 2000: every copy ties with its original in every round, and once the 40 are used up
    all running minima are 0, whose first arg-max is index 0 -- as numpy gives"""
    pts, first, want, claims = so.fps_repeated(17, 2, 40, 2000, 64)
    assert claims["used"] == 40 and claims["tie"] == 63 and claims["slot"] >= 40 and not want[:, 40:].any()
    got = _ops().fps(dev(pts), dev(first), 64)
    _same_indices(got, want, "fps repeated")
    assert not host(got)[:, 40:].any()


def test_fps_refuses_what_it_cannot_sample():
    ops = _ops()
    pts, first = torch.zeros(2, 3, 70, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV)
    for k in (71, 0):
        with pytest.raises(RuntimeError):
            ops.fps(pts, first, k)
    with pytest.raises(RuntimeError):
        ops.fps(torch.zeros(2, 3, 16385, device=DEV), first, 4)


# =============================================================================================== usip_nms_f32
def _nms_check(kp, sigma, radius, what):
    """runs the kernel, compares order, count and the zero tail with the reference -> (count, claims)"""
    want_order, want_count, claims = so.nms_reference(kp, sigma, radius)
    order, count = _ops().nms(dev(kp), dev(sigma), float(radius))
    order, count = host(order), host(count)
    assert order.dtype == np.int32 and count.dtype == np.int32
    assert np.array_equal(count, want_count), "%s: kept %s, want %s" % (what, count.tolist(), want_count.tolist())
    bad = np.argwhere(order != want_order)                                  # order[count:] stays zero: want_order has it so
    assert len(bad) == 0, "%s: %d differ, first at %s: got %d, want %d" % (
        what, len(bad), tuple(bad[0]), order[tuple(bad[0])], want_order[tuple(bad[0])])
    for b in range(len(count)):
        assert not order[b, count[b]:].any()
    return count, claims


@pytest.mark.parametrize("name", sorted(so.NMS_CASES))
def test_nms_on_a_lattice_with_shared_sigmas(name):
    """sigmas drawn from five values: nearly every pick is a tie, settled by the lowest index in the lane butterfly and in
    the wave merge; thousands of pairs sit at d == radius, where `d > radius survives` must suppress"""
    args, floors = so.NMS_CASES[name]
    kp, sigma = so.nms_lattice(*args[:4])
    count, claims = _nms_check(kp, sigma, args[4], "nms " + name)
    assert claims["at_radius"] >= floors[0] and claims["tie"] >= floors[1] and claims["wave"] >= floors[2], (claims, floors)


def test_nms_equality_with_the_radius_decides():
    """the same cloud at r = 1 and at the float32 just below 1: the kept count differs, so d == r pairs are in play"""
    args = so.NMS_CASES["m1024_r1"][0]
    kp, sigma = so.nms_lattice(*args[:4])
    ops = _ops()
    at_one = host(ops.nms(dev(kp), dev(sigma), 1.0)[1])
    below = host(ops.nms(dev(kp), dev(sigma), so.BELOW_ONE)[1])
    assert (below != at_one).all() and (below == 1024).all() and (at_one < 700).all()


@pytest.mark.parametrize("M", [65, 1024])
def test_nms_with_equal_sigmas_picks_by_ascending_index(M):
    kp, _ = so.nms_lattice(25, 2, M, 11)
    sigma = np.full((2, M), 0.75, np.float32)
    count, claims = _nms_check(kp, sigma, 1.0, "nms equal sigmas")
    assert claims["tie"] >= count.min() - 1 >= 30 and claims["wave"] >= 1
    order = host(_ops().nms(dev(kp), dev(sigma), 1.0)[0])
    for b in range(2):
        kept = order[b, :count[b]]
        assert kept[0] == 0 and (np.diff(kept) > 0).all()                  # greedy in index order


def test_nms_of_identical_points_keeps_one():
    kp = np.full((3, 3, 1000), 2.5, np.float32)
    sigma = np.random.default_rng(26).uniform(0.1, 1.0, (3, 1000)).astype(np.float32)
    sigma[1] = 0.5                                                          # and with every sigma equal: index 0
    count, _ = _nms_check(kp, sigma, 0.5, "nms identical points")
    assert count.tolist() == [1, 1, 1]
    order = host(_ops().nms(dev(kp), dev(sigma), 0.5)[0])
    assert order[:, 0].tolist() == [int(np.argmin(sigma[0])), 0, int(np.argmin(sigma[2]))]


def test_nms_with_an_infinite_sigma_among_finite_ones():
    """+inf is the value the kernel gives to dead lanes: a LIVE point that carries it must still be picked, last"""
    args = so.NMS_CASES["m65"][0]
    kp, sigma = so.nms_lattice(*args[:4])
    sigma = sigma.copy()
    sigma[:, 3] = np.inf
    sigma[1, 64] = np.inf                                                   # the lone lane of the second wave
    kp = kp.copy()
    kp[:, :, 3] = 100.0                                                     # far from everything: nobody suppresses it
    kp[1, :, 64] = -100.0
    count, _ = _nms_check(kp, sigma, 1.0, "nms inf sigma")
    order = host(_ops().nms(dev(kp), dev(sigma), 1.0)[0])
    assert order[0, count[0] - 1] == 3 and order[1, count[1] - 2:count[1]].tolist() == [3, 64]


def test_nms_refuses_more_than_1024_keypoints():
    with pytest.raises(RuntimeError):
        _ops().nms(torch.zeros(2, 3, 1025, device=DEV), torch.ones(2, 1025, device=DEV), 1.0)


# =============================================================================================== usip_som_assign_f32
@pytest.mark.parametrize("name", sorted(so.SOM_CASES))
def test_som_assign_on_a_lattice_takes_the_first_nearest_node(name):
    args, floor = so.SOM_CASES[name]
    x, node, want, claims = so.som_lattice(*args)
    assert claims["tied"] >= floor, claims
    _same_indices(_ops().som_assign(dev(x), dev(node)), want, "som_assign " + name)


def test_som_assign_refuses_a_node_table_beyond_the_lds():
    with pytest.raises(RuntimeError):
        _ops().som_assign(torch.zeros(2, 3, 300, device=DEV), torch.zeros(2, 3, 5462, device=DEV))


@pytest.mark.parametrize("M", [8, 9, 33])
def test_som_assign_midway_between_two_nodes(M):
    """a point midway between the two nodes of one packed pair, between neighbouring pairs, and (odd M) between the last
    pair and the scalar tail goes to the LOWER node; a point on a node goes to it"""
    x, node, want, tied = so.som_hand_placed(M)
    ref, ref_tied = so.som_assign_f32(x, node)
    assert np.array_equal(ref, want) and np.array_equal(ref_tied, tied) and tied[:, :M - 1].all()
    assert np.array_equal(want[0, :M - 1], np.arange(M - 1))
    _same_indices(_ops().som_assign(dev(x), dev(node)), want, "som_assign midpoints")


@pytest.mark.parametrize("M", [8, 9])
def test_som_assign_with_the_same_node_twice(M):
    """FPS on a cloud padded by repetition hands over duplicate nodes: the first copy wins, within a pair, across pairs
    and against the last place"""
    x, node, want, tied = so.som_hand_placed(M, duplicates=True)
    ref, _ = so.som_assign_f32(x, node)
    assert np.array_equal(ref, want) and want[0, [1, 5, M - 1]].tolist() == [0, 2, 3] and tied[0, [1, 5, M - 1]].all()
    _same_indices(_ops().som_assign(dev(x), dev(node)), want, "som_assign duplicate nodes")


# =============================================================================================== usip_som_cluster(_csr)_f32
WORST = {}


def _cluster_check(x, min_idx, M, kind, t_idx=None):
    """scan and segment walk against the exact reference: counts exactly, means within the derived bound, the decentred
    cloud bit for bit from the kernel's own means.  t_idx: the device tensor to hand over as min_idx."""
    ops = _ops()
    want_mean, want_count, bound = so.som_cluster_exact(x, min_idx, M)
    tx = dev(x)
    t_idx = dev(min_idx) if t_idx is None else t_idx
    csr = ops.csr_by_index(t_idx, M)
    for path, kw in (("scan", {}), ("csr", {"csr": csr})):
        mean, count, dec = ops.som_cluster(tx, t_idx, M, **kw)
        mean, count, dec = host(mean), host(count), host(dec)
        assert mean.dtype == np.float32 and count.dtype == np.int32 and dec.dtype == np.float32
        assert np.array_equal(count, want_count), (path, kind)
        err = np.abs(mean.astype(np.float64) - want_mean.astype(np.float64))
        ratio = float((err / bound).max())
        WORST[(kind, path)] = max(WORST.get((kind, path), 0.0), ratio)
        print("ratio cluster_mean %-10s %-4s N=%d M=%d  %.3f" % (kind, path, x.shape[2], M, ratio))
        assert np.isfinite(mean).all() and ratio <= 1.0, "%s %s: worst err / bound = %.3f" % (kind, path, ratio)
        assert not mean[np.broadcast_to((want_count == 0)[:, None, :], mean.shape)].any()          # no member: mean 0
        assert np.array_equal(dec.view(np.int32), so.som_decenter_f32(x, mean, min_idx).view(np.int32)), (path, kind)


CLUSTER_CASES = [(N, M, kind) for N, M in so.CLUSTER_SHAPES for kind in so.CLUSTER_KINDS
                 if not (kind == "empty_node" and M == 1)]                 # one node cannot be the empty one


@pytest.mark.parametrize("N,M,kind", CLUSTER_CASES)
def test_som_cluster_means_are_the_rounded_exact_means(N, M, kind):
    x, min_idx, claims = so.cluster_case(N, M, kind)
    if kind == "cancel":
        assert claims["cancel"] >= so.CANCEL_FLOOR
    if kind == "empty_node":
        assert claims["empty"] == 0
    if kind == "one_node":
        assert claims["all"] == 1
    _cluster_check(x, min_idx, M, kind)


@pytest.mark.parametrize("kind", ["normal", "cancel"])
def test_som_cluster_with_min_idx_four_bytes_into_its_storage(kind):
    """N % 4 == 0 but the index rows are not 16-byte aligned: the scan must fall back to its scalar loop, not read int4s"""
    N, M = 1024, 33
    x, min_idx, _ = so.cluster_case(N, M, kind)
    store = torch.zeros(2 * N + 1, dtype=torch.int32, device=DEV)
    view = store[1:].view(2, N)
    view.copy_(dev(min_idx))
    assert view.is_contiguous() and view.data_ptr() % 16 == 4 and (view.data_ptr() + 4 * N) % 16 == 4
    _cluster_check(x, min_idx, M, kind, t_idx=view)


# =============================================================================================== usip_knn_f32
KNN_CASES = [(N, K) for N in sorted(so.KNN_SIDES) for K in (1, 5, 64) + ((N,) if 64 < N <= 257 else ())]


@pytest.mark.parametrize("N,K", KNN_CASES)
def test_knn_on_a_lattice_puts_the_lower_index_first(N, K):
    """full index equality with the stable sort of the distance rows, NO mask: ties inside the K picks fix their order,
    ties across the K-th place fix the selection.  N = 256|257 and 512|513: 4, 8 and 16 slots per lane; K = N up to
    N = 257 (at N = 64, K = 64 is K = N)."""
    q, db, dist = so.knn_case(N)
    c, (inside, across) = so.knn_tie_claims(dist, K), so.knn_floors(N, K)
    assert c["inside"] >= inside and c["across"] >= across, c
    want, _ = so.knn_reference(q, db, K)
    _same_indices(_ops().knn(dev(q), dev(db), K), want.astype(np.int32), "knn N=%d K=%d" % (N, K))


def test_knn_refuses_what_it_cannot_hold():
    ops = _ops()
    q = torch.zeros(2, 3, 8, device=DEV)
    with pytest.raises(RuntimeError):
        ops.knn(q, torch.zeros(2, 3, 1025, device=DEV), 4)
    with pytest.raises(RuntimeError):
        ops.knn(q, torch.zeros(2, 3, 64, device=DEV), 65)


# =============================================================================================== usip_knn_points_f32
@pytest.mark.parametrize("N", [256, 300])
def test_knn_points_at_its_limit_of_256_neighbours(N):
    """K = 256: a wave's quota is a full 64 lanes; N = 256: every point is a neighbour, N = 300: lattice ties across the
    256-th place"""
    q, db, dist = so.knn_lattice(60 + N, 2, 5, N, 7)
    K = 256
    c = so.knn_tie_claims(dist, K)
    assert c["inside"] == c["rows"] == 10 and (N == 256 or c["across"] >= 5), c
    want, _ = so.knn_reference(q, db, K)
    _same_indices(_ops().knn_points(dev(q), dev(db), K), want.astype(np.int32), "knn_points N=%d" % N)


def test_knn_points_refuses_what_it_cannot_hold():
    ops = _ops()
    q = torch.zeros(2, 3, 4, device=DEV)
    with pytest.raises(RuntimeError):
        ops.knn_points(q, torch.zeros(2, 3, 300, device=DEV), 257)
    with pytest.raises(RuntimeError):
        ops.knn_points(q, torch.zeros(2, 3, 16385, device=DEV), 64)
