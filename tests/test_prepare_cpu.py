"""Host twins of the f-7 scan preparation (csrc/prepare_cpu.cpp over csrc/prepare_math.h) against the independent
restatement of tests/prepare_oracle.py (cKDTree neighbours, numpy.linalg.eigh -- not the product's Jacobi --, a plain numpy
grid).  The device runs the same header; tests/test_prepare_gpu.py holds it to these twins bit for bit.

Input: the surface scene scene(seed=7, n=20000) -- no K-th / (K+1)-th distance tie, no duplicate points.

Tolerances on a normal, derived: both sides are float64; an eigenvector's error is bounded by |E| / gap with |E| a few eps
of |C|, so with the gap ratio (l1 - l0) / l2 at the leave-out cap of 1e-3 a component agrees to a few times 2.2e-16 / 1e-3,
about 2e-12.  The first bound asserted was 1e-10 (room for the solver's constant); measured, the host twin is at 1.8e-14 on
the 20 000 points of the surface scene (smallest gap ratio met: 1.7e-3) and at 3.1e-14 on the 119 768 points of the ring scan
(gap ratios down to the cap; the device gives the same bits, tests/test_prepare_gpu.py), so the asserted bound is tightened
to 1e-13, 3x the larger of the two.  Curvature: 1e-12 absolute (an eigenvalue's error is a few eps of the trace; measured
3.5e-16 and 4.4e-16).  A point is left out when the oracle's gap ratio is below 1e-3, its flip product below 1e-9 in
magnitude or its two largest |normal| components within 1e-9;
at most 1 % may be (0 of 20 000 are)."""
import sys

import numpy as np
import pytest

import prepare_oracle as po
from conftest import GOLDEN
from usip_amd import pairs, prepare

sys.path.insert(0, GOLDEN)
import make_tile_walk_golden as tw  # noqa: E402   (the cases of tests/golden/tile_walk_parent_bits.npz and how they are stored)

K = 9
VIEW = (0.0, 0.0, 1.0)
TOL_N, TOL_C = 1e-13, 1e-12


@pytest.fixture(scope="module")
def scan():
    return po.scene(7, 20000)


@pytest.fixture(scope="module")
def twin(scan):
    n64, idx, n32 = prepare.normals_cpu(scan, None, K, VIEW, num_threads=4)
    return n64, idx, n32


def test_neighbours_equal_the_oracle_and_do_not_depend_on_threads(scan, twin):
    want, d2 = po.neighbours(scan, K)
    assert not po.kth_tie(d2, K).any()                       # the scene has no tie: the oracle's order is THE order
    assert np.array_equal(twin[1], want)
    one, five = prepare.knn_cpu(scan[:3000], K, 1), prepare.knn_cpu(scan[:3000], K, 5)
    assert np.array_equal(one, five) and np.array_equal(one, po.neighbours(scan[:3000], K)[0])


def test_tie_rule_and_exclusion_by_index():
    """Duplicates and equidistant points: ascending (d2, index), the point itself left out by INDEX -- its duplicate stays."""
    pts = np.array([[0, 0, 0], [0, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [5, 5, 5], [0, 0, 0], [0, -1, 0]], np.float32)
    xyzi = np.concatenate((pts, np.zeros((len(pts), 1), np.float32)), 1)
    for k in (1, 2, 3, 7):
        got = prepare.knn_cpu(xyzi, k)
        assert np.array_equal(got, po.neighbours_brute(xyzi, k)), k
    got = prepare.knn_cpu(xyzi, 3)
    assert got[0].tolist() == [1, 6, 2]                      # the duplicates first (lower index first), then the first of
    assert got[1].tolist() == [0, 6, 2]                      # the four points at distance 1
    assert got[6].tolist() == [0, 1, 2]
    assert got[2].tolist() == [0, 1, 6]
    with pytest.raises(RuntimeError):
        prepare.knn_cpu(xyzi, 8)                             # n >= K + 1
    with pytest.raises(RuntimeError):
        prepare.knn_cpu(xyzi, 17)


def test_normals_and_curvature_match_eigh(scan, twin):
    n64, idx, n32 = twin
    o = po.normals(scan, idx, VIEW)
    keep = po.comparable(o)
    print("left out: %d of %d (gap < 1e-3: %d); smallest gap ratio kept %.3e" % (
        (~keep).sum(), len(keep), (o["gap"] < 1e-3).sum(), o["gap"][keep].min()))
    assert (~keep).mean() <= 0.01
    assert np.isfinite(n64).all() and np.isfinite(n32).all()
    assert np.abs(np.linalg.norm(n64[:, :3], axis=1) - 1.0).max() <= 1e-12
    err_n = np.abs(n64[keep, :3] - o["normal"][keep]).max()
    err_c = np.abs(n64[:, 3] - o["curvature"]).max()
    print("normal: max component error %.3e (bound %.1e); curvature: %.3e (bound %.1e)" % (err_n, TOL_N, err_c, TOL_C))
    assert err_n <= TOL_N
    assert err_c <= TOL_C
    assert np.array_equal(n32, n64.astype(np.float32))
    assert (n64[:, 3] >= -1e-15).all() and (n64[:, 3] <= 1.0 / 3.0 + 1e-12).all()


def test_grid_cells_members_and_rows(scan, twin):
    n64 = twin[0]
    rows, keys, perm, start = prepare.grid_cpu(scan, n64, 0.2)
    o = po.grid(scan, n64, 0.2)
    assert len(keys) == len(o["keys"]) == rows.shape[0] and np.array_equal(keys, o["keys"])
    assert all(np.array_equal(perm[start[c]:start[c + 1]], o["members"][c]) for c in range(len(keys)))
    ulp = po.ulp_apart(rows, o["rows"])
    print("cells %d, largest cell %d, rows differ by at most %.1f float32 ulp, smallest mean-normal norm %.4f" % (
        len(keys), np.diff(start).max(), ulp.max(), o["normal_len"].min()))
    assert ulp.max() <= 1.0
    assert np.abs(np.linalg.norm(rows[:, 3:6], axis=1) - 1.0).max() < 1e-6


def test_degenerate_cases():
    # n = K + 1 with every point the same: a zero trace -> curvature 0, normal (0, 0, 1) before the flip; z = 3 lies above
    # the view point, so the flip turns it down
    same = np.tile(np.array([[1.0, 2.0, 3.0, 0.5]], np.float32), (4, 1))
    n64, idx, _ = prepare.normals_cpu(same, None, 3, VIEW)
    assert np.array_equal(idx, [[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]])
    assert np.array_equal(n64, np.tile([[0.0, 0.0, -1.0, 0.0]], (4, 1)))
    below = same.copy()
    below[:, 2] = -3.0
    assert np.array_equal(prepare.normals_cpu(below, None, 3, VIEW)[0], np.tile([[0.0, 0.0, 1.0, 0.0]], (4, 1)))
    # a zero mean normal takes the first member's; a single-member cell is the point itself
    pts = np.array([[0.01, 0.01, 0.01, 0.2], [0.05, 0.05, 0.05, 0.4], [1.0, 1.0, 1.0, 0.6]], np.float32)
    nrm = np.array([[0, 0, 1, 0.1], [0, 0, -1, 0.3], [0, 1, 0, 0.25]], np.float64)
    rows, keys, perm, start = prepare.grid_cpu(pts, nrm, 0.2)
    assert rows.shape == (2, 8) and start.tolist() == [0, 2, 3] and perm.tolist() == [0, 1, 2]
    assert rows[0, 3:6].tolist() == [0.0, 0.0, 1.0]
    assert po.ulp_apart(rows[0, [0, 6, 7]], np.array([0.03, 0.2, 0.3], np.float32)).max() <= 1.0
    assert np.array_equal(rows[1], np.array([1, 1, 1, 0, 1, 0, 0.25, 0.6], np.float32))
    # a plane of 10 points, n = K + 1: the normal is the plane's, turned towards the view point above it
    rng = np.random.default_rng(0)
    plane = np.concatenate((rng.uniform(-1, 1, (10, 2)), np.full((10, 1), -2.0), np.zeros((10, 1))), 1).astype(np.float32)
    n64 = prepare.normals_cpu(plane, None, 9, VIEW)[0]
    assert np.abs(n64[:, :3] - [0.0, 0.0, 1.0]).max() < 1e-12 and np.abs(n64[:, 3]).max() < 1e-15


def test_frame_and_max_rows(scan):
    small = scan[:6000]
    a = np.deg2rad(30.0)
    R = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]]) @ \
        np.array([[1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]])
    frame = np.concatenate((R, [[0.5], [-2.0], [1.5]]), 1)
    plain = prepare.prepare_cpu(small, K)
    moved = prepare.prepare_cpu(small, K, frame=frame)
    assert moved.shape == plain.shape and moved.dtype == np.float32
    want_xyz = plain[:, :3].astype(np.float64) @ R.T + frame[:, 3]
    want_n = plain[:, 3:6].astype(np.float64) @ R.T
    assert po.ulp_apart(moved[:, :3], want_xyz.astype(np.float32)).max() <= 1.0
    assert np.abs(moved[:, 3:6] - want_n).max() <= 1e-6
    assert np.array_equal(moved[:, 6:], plain[:, 6:])
    # ... and the same transform applied to the INPUT gives the same normals up to the float32 rounding of the moved
    # points (the grid's cells differ, so this is held per point, before the grid)
    n_in = prepare.normals_cpu(small, None, K, VIEW)[0]
    turned = small.copy()
    turned[:, :3] = (small[:, :3].astype(np.float64) @ R.T + frame[:, 3]).astype(np.float32)
    view = R @ np.asarray(VIEW) + frame[:, 3]
    idx = prepare.knn_cpu(small, K)                          # (the same neighbours: a near-tie may swap under the rounding)
    n_out = prepare.normals_cpu(turned, idx, K, view)[0]
    o = po.normals(small, idx, VIEW)
    keep = po.comparable(o, gap=1e-2, flip=1e-3, top2=0.0)
    same_sign = np.sign((n_in[:, :3] @ R.T * n_out[:, :3]).sum(1))
    dev = np.abs(n_in[keep, :3] @ R.T - n_out[keep, :3] * same_sign[keep, None]).max()
    print("normals of the moved input against the moved normals: %.3e" % dev)
    assert dev <= 1e-2                                       # float32 rounding of ~20 m coordinates (1e-6) over a 1e-2 gap
    # max_rows: exactly that many distinct rows, a function of (seed, scan_id)
    cut = prepare.prepare_cpu(small, K, max_rows=1000, seed=3, scan_id=5)
    again = prepare.prepare_cpu(small, K, max_rows=1000, seed=3, scan_id=5)
    other = prepare.prepare_cpu(small, K, max_rows=1000, seed=3, scan_id=6)
    assert cut.shape == (1000, 8) and np.array_equal(cut, again) and not np.array_equal(cut, other)
    pos = [np.flatnonzero((plain == r).all(1)) for r in cut]
    assert all(len(p) >= 1 for p in pos)
    first = np.array([p[0] for p in pos])
    assert len(np.unique(first)) == 1000 and (np.diff(first) > 0).all()      # distinct rows, ascending row order
    assert prepare.prepare_cpu(small, K, max_rows=10 ** 6).shape == plain.shape


def test_prepared_rows_feed_the_pair_builder(scan):
    rows = prepare.prepare_cpu(scan, K)
    assert rows.ndim == 2 and rows.shape[1] == 8 and rows.dtype == np.float32 and np.isfinite(rows).all()
    recipe = pairs.PairRecipe(N=4096, M=64, Cs=4, n_sub=1365)
    batch, picked, _ = pairs.build_cpu(recipe, [rows, rows[::2].copy()], [0, 1], 2, seed=1, step=0)
    assert batch["src_pc"].shape == (2, 3, 4096) and batch["src_sn"].shape == (2, 4, 4096)
    assert all(np.isfinite(v).all() for v in batch.values())
    assert picked.min() >= 0 and picked[:, 0].max() < len(rows)


def test_bin_files_round_trip(tmp_path, scan):
    f = tmp_path / "000000.bin"
    scan.tofile(f)
    assert np.array_equal(prepare.load_velodyne_bin(f), scan)
    rows = prepare.prepare_cpu(scan[:2000], K)
    prepare.save_test_bin(tmp_path / "out.bin", rows)
    assert np.array_equal(np.fromfile(tmp_path / "out.bin", np.float32).reshape(-1, 6), rows[:, :6])


@pytest.mark.parametrize("name", tw.SCANS)
def test_neighbours_give_the_bits_pinned_before_the_thread_split_was_shared(name):
    """tests/golden/tile_walk_parent_bits.npz: K = 1, 9, 16 on 255, 256, 257 and 515 rows and on a constant-x run."""
    tw.check("knn-" + name, {"idx%d" % k: tw.knn_host(name, k) for k in tw.KNN_K}, "host twin")
