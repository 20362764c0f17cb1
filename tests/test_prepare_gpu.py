"""The f-7 scan-preparation kernels on the MI355X (csrc/prepare.hip) against the library's host twins, which run the same
header (csrc/prepare_math.h), and against the independent oracle (tests/prepare_oracle.py).  Device and host twin are held
to equality as bit patterns: neighbour indices, the float64 normals and curvature (Jacobi, sqrt and division in float64:
the f-6 tests set the precedent on this chip), cell keys, the number of cells and the float32 [m,8] rows.  Because the twin
walks all pairs, this is also what proves the device's pruned walk exact.

Inputs: the surface scene scene(seed=7, n=20000) and the full ring scan ring_scan(seed=3): 119 768 points, 23 079 occupied
cells, no K-th / (K+1)-th distance tie (0 points within 1e-12 relative), eigen-gap ratio below 1e-3 for 411 points (0.34 %)
-- re-checked on a CPU with this file's generator.  Bounds against the oracle: tests/test_prepare_cpu.py (the host twin on
the ring scan is at 3.1e-14 on a normal's components and 4.4e-16 on the curvature)."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import prepare_oracle as po
import test_prepare_cpu as host
from conftest import ROOT
from usip_amd import pairs, prepare, synth

pytestmark = pytest.mark.gpu
K, VIEW, LEAF = host.K, host.VIEW, 0.2
DEV = "cuda:0"


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def device_stages(scan, k=K):
    prep = prepare.ScanPreparer(DEV, k=k, leaf=LEAF, viewpoint=VIEW)
    pts = torch.from_numpy(scan).to(DEV)
    n64, idx = prep.normals(pts)
    rows, keys, perm, start = prep.grid(pts, n64)
    return dict(idx=idx, n64=n64, rows=rows, keys=keys, perm=perm, start=start)


def host_stages(scan, k=K, threads=16):
    n64, idx, _ = prepare.normals_cpu(scan, None, k, VIEW, num_threads=threads)
    rows, keys, perm, start = prepare.grid_cpu(scan, n64, LEAF)
    return dict(idx=idx, n64=n64, rows=rows, keys=keys, perm=perm, start=start)


@pytest.fixture(scope="module")
def ring():
    scan = po.ring_scan(3)
    return scan, device_stages(scan), host_stages(scan)


def assert_same_bits(d, h):
    for k in ("idx", "n64", "keys", "perm", "start", "rows"):
        a, b = bits(d[k]), bits(h[k])
        assert a.shape == b.shape and a.dtype == b.dtype, (k, a.shape, b.shape, a.dtype, b.dtype)
        bad = np.flatnonzero((a != b).reshape(len(a), -1).any(1)) if a.size else []
        assert len(bad) == 0, "%s: %d rows differ, first %s" % (k, len(bad), bad[:5])


@pytest.mark.parametrize("k", [1, 9, 16])
def test_device_equals_host_twin_on_the_surface_scene(k):
    scan = po.scene(7, 20000)
    assert_same_bits(device_stages(scan, k), host_stages(scan, k))


def test_device_equals_host_twin_on_the_ring_scan(ring):
    scan, d, h = ring
    assert len(scan) == 119768 and d["rows"].shape == (23079, 8)
    assert_same_bits(d, h)


def test_small_and_ragged_scans_equal_the_host_twin():
    """n = K + 1, one partly filled tile, a tile boundary, duplicates and equidistant points (the tie rule on ORIGINAL
    indices although the device walks the scan in x order)."""
    rng = np.random.default_rng(5)
    for n in (K + 1, 255, 256, 257, 1000):
        scan = rng.normal(size=(n, 4)).astype(np.float32)
        scan[n // 2:, :3] = np.round(scan[n // 2:, :3] * 2) / 2          # a lattice: many exact ties and duplicates
        assert_same_bits(device_stages(scan), host_stages(scan, threads=2))
    prep = prepare.ScanPreparer(DEV, k=K)
    with pytest.raises(RuntimeError):
        prep.normals(np.zeros((K, 4), np.float32))                       # n >= K + 1


def test_device_against_the_oracle_on_the_ring_scan(ring):
    scan, d, _ = ring
    idx, n64 = d["idx"].cpu().numpy(), d["n64"].cpu().numpy()
    want, d2 = po.neighbours(scan, K, workers=16)
    tie = po.kth_tie(d2, K)
    print("K-th distance ties within 1e-12 relative: %d of %d" % (tie.sum(), len(tie)))
    assert np.array_equal(idx[~tie], want[~tie])
    o = po.normals(scan, idx, VIEW)
    keep = po.comparable(o) & ~tie
    print("left out: %d of %d (%.2f %%; gap ratio < 1e-3: %d)" % ((~keep).sum(), len(keep), 100 * (~keep).mean(),
                                                                  (o["gap"] < 1e-3).sum()))
    assert (~keep).mean() <= 0.01
    assert np.isfinite(n64).all() and np.isfinite(d["rows"].cpu().numpy()).all()
    assert np.abs(np.linalg.norm(n64[:, :3], axis=1) - 1.0).max() <= 1e-12
    err_n = np.abs(n64[keep, :3] - o["normal"][keep]).max()
    err_c = np.abs(n64[:, 3] - o["curvature"]).max()
    print("normal: max component error %.3e (bound %.1e); curvature: %.3e (bound %.1e)" % (err_n, host.TOL_N, err_c, host.TOL_C))
    assert err_n <= host.TOL_N and err_c <= host.TOL_C
    g = po.grid(scan, n64, LEAF)
    assert np.array_equal(d["keys"].cpu().numpy(), g["keys"])
    assert po.ulp_apart(d["rows"].cpu().numpy(), g["rows"]).max() <= 1.0


def test_the_synthetic_scan_of_the_examples_is_the_test_input():
    assert np.array_equal(synth.make_ring_scan(3), po.ring_scan(3))


def test_two_calls_agree_and_a_side_stream_is_ordered(ring):
    scan, d, _ = ring
    prep = prepare.ScanPreparer(DEV, k=K, leaf=LEAF, viewpoint=VIEW)
    again = prep(scan)
    assert np.array_equal(bits(again), bits(d["rows"])) and np.array_equal(bits(prep(scan)), bits(again))
    # the scan is produced on the side stream right before the call: only stream order makes the result right
    base = torch.from_numpy(scan).to(DEV)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(DEV)
    with torch.cuda.stream(side):
        pts = base
        for _ in range(50):                                              # work ahead of the call on the same stream;
            pts = pts * 1.0                                              # (x * 1.0 is exact: pts equals base bit for bit)
        rows = prep(pts)
        n64, idx = prep.normals(pts)
    side.synchronize()
    assert np.array_equal(bits(rows), bits(d["rows"]))
    assert np.array_equal(bits(n64), bits(d["n64"])) and np.array_equal(bits(idx), bits(d["idx"]))


def test_frame_and_max_rows_on_the_device():
    scan = po.scene(7, 20000)
    frame = np.array([[0.0, -1.0, 0.0, 0.3], [0.0, 0.0, -1.0, -0.1], [1.0, 0.0, 0.0, 0.2]])
    want = prepare.prepare_cpu(scan, K, LEAF, VIEW, frame=frame, max_rows=5000, seed=4, scan_id=11, num_threads=16)
    got = prepare.ScanPreparer(DEV, k=K, leaf=LEAF, viewpoint=VIEW, frame=frame, max_rows=5000, seed=4)(scan, scan_id=11)
    assert got.shape == (5000, 8) and got.dtype == torch.float32 and got.is_cuda
    assert po.ulp_apart(got.cpu().numpy(), want).max() <= 1.0           # (the frame is a torch matmul on either side)


def test_bank_from_device_rows_feeds_the_pair_builder():
    prep = prepare.ScanPreparer(DEV, k=K, leaf=LEAF)
    rows = [prep(po.scene(seed, 20000), scan_id=i) for i, seed in enumerate((7, 8, 9))]
    bank = pairs.ScanBank.from_device_rows(rows)
    ref = pairs.ScanBank([r.cpu().numpy() for r in rows], DEV)
    assert bank.num_scans == 3 and bank.min_rows == ref.min_rows and bank.row_len == 8
    assert np.array_equal(bank.offsets_host, ref.offsets_host) and torch.equal(bank.offsets, ref.offsets)
    assert np.array_equal(bits(bank.rows), bits(ref.rows))
    near = pairs.ScanBank.from_device_rows(rows, radius_threshold=15.0)
    near_ref = pairs.ScanBank([r.cpu().numpy() for r in rows], DEV, radius_threshold=15.0)
    assert np.array_equal(near.offsets_host, near_ref.offsets_host) and np.array_equal(bits(near.rows), bits(near_ref.rows))
    recipe = pairs.PairRecipe(N=8192, M=128, Cs=4, n_sub=2730)
    ids = [2, 0, 1, 1]
    got = pairs.PairBuilder(bank, recipe, 4, DEV, seed=6).build(ids, 3)
    want = pairs.PairBuilder(ref, recipe, 4, DEV, seed=6).build(ids, 3)
    shapes = dict(src_pc=(4, 3, 8192), src_sn=(4, 4, 8192), src_node=(4, 3, 128), dst_pc=(4, 3, 8192), dst_sn=(4, 4, 8192),
                  dst_node=(4, 3, 128), R=(4, 3, 3), scale=(4,), shift=(4, 3, 1))
    for k, shape in shapes.items():
        assert tuple(got[k].shape) == shape and bool(torch.isfinite(got[k]).all()), k
        assert torch.equal(got[k], want[k]), k
    with pytest.raises(ValueError):
        pairs.ScanBank.from_device_rows([rows[0][:, :6]])


def test_prepare_example_feeds_the_training_example(tmp_path):
    scans = tmp_path / "prepared"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "prepare_scans.py"), "--make-synthetic", str(scans),
                        "--test-bin"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    print(line)
    assert line["scans"] >= 8 and 0 < line["rows_out"] < line["points_in"]
    first = np.load(scans / "000000.npy")
    assert first.ndim == 2 and first.shape[1] == 8 and first.dtype == np.float32
    assert np.array_equal(np.fromfile(scans / "000000.bin", np.float32).reshape(-1, 6), first[:, :6])
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_detector_scans.py"), "--scans", str(scans),
                        "--steps", "5", "--out", str(tmp_path / "det.pth")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    losses = [float(ln.split()[3]) for ln in r.stdout.splitlines() if ln.startswith("step")]
    assert losses and all(math.isfinite(v) for v in losses)


@pytest.mark.parametrize("name", host.tw.SCANS)
def test_neighbours_on_the_device_give_the_pinned_parent_bits(name):
    """tests/golden/tile_walk_parent_bits.npz through scan_knn_kernel<K> over csrc/tile_walk.h's tiles and reduction."""
    host.tw.check("knn-" + name, {"idx%d" % k: host.tw.knn_device(name, k, DEV) for k in host.tw.KNN_K}, "device")
