"""Bits of the x-sorted neighbour searches' host twins pinned at one commit: tests/golden/tile_walk_parent_bits.npz.

The device kernels are held to the host twins (tests/test_fragments_gpu.py, tests/test_icp_gpu.py, tests/test_prepare_gpu.py),
but twin and device share the *_math.h headers and could drift together.  This fixture holds what the twins computed at the
commit BEFORE the fragment bank view (csrc/bank.h), the outward tile walk (csrc/tile_walk.h) and the twins' thread split
(csrc/host_split.h) became one each: tests/test_fragments_cpu.py, tests/test_icp_cpu.py and tests/test_prepare_cpu.py hold
today's twins to it bit for bit, the three GPU files the device.

Inputs are not stored: they come from the tests' seeded generators (tests/fragments_oracle.py, tests/icp_oracle.py,
fragments.synthetic_scene, the scans below), and the fixture holds a SHA-256 of them, so a generator that has moved fails the
test instead of moving the expectation.

  overlap-*     (ratio, hits) of overlap_ratio_cpu: the exact lattice, small and large, both ways round; the constant-x
                walls beside 300-, 512- and 0-point fragments; the walls' fragments 50 m apart to either side (the binary
                search ends at lo == nd with the start tile clamped, or at 0)
  icp-<name>    every name of icp_oracle.NAMES: one nearest pass (idx, d2) under the start pose, and icp_refine_cpu's Rt,
                iterations, converged, rmse, hits, ratio and the trim's cut (d2*, i*) of every pass
  knn-<n>       scan_knn's indices at K = 1, 9, 16 on scans of 255, 256, 257 and 515 rows (half of each on a half-unit lattice:
                exact ties and duplicates) and on a 515-row scan of constant x (a run longer than two tiles)
  pairs-<reg>   every key of register_pairs_cpu for "ransac" and "fgr" with refine and dense_radius set, on
                synthetic_scene(fragments=3, points=2000, dim=32)
Float outputs are stored as their bit patterns, integers and booleans as they are.

    python tests/golden/make_tile_walk_golden.py       (regenerating it moves the pin: do that only on purpose)
"""
import functools
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))                              # the oracles' generators

PATH = os.path.join(HERE, "tile_walk_parent_bits.npz")
OVERLAP = ("lattice_small", "lattice_large", "walls", "apart")
KNN_K = (1, 9, 16)
SCANS = {"255": 255, "256": 256, "257": 257, "515": 515, "515_constant_x": 515}
REGISTRATORS = ("ransac", "fgr")
SCENE = dict(seed=0, fragments=3, points=2000, dim=32)
THREADS = 8


def bits(a):
    """An output as the fixture stores it: a float as its bit pattern, everything else as it is."""
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def sha(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return np.frombuffer(h.digest(), np.uint8)


# ------------------------------------------------------------------------------------------------ overlap
@functools.lru_cache(maxsize=None)
def overlap_case(name):
    """-> (clouds, frag1, frag2, Rt f64 [P,3,4], radius)"""
    import fragments_oracle as fo
    if name.startswith("lattice_"):
        a, b, Rt, _, _ = fo.lattice_pair(name[len("lattice_"):])
        return [a, b], np.array([0, 1], np.int32), np.array([1, 0], np.int32), np.stack([Rt, fo.inverse_pose(Rt)]), \
            fo.LATTICE_RADIUS
    clouds, Rt, _ = fo.wall_rooms()
    if name == "walls":
        f1, f2 = np.array([0, 1, 2, 0, 0, 3, 4, 1], np.int32), np.array([1, 0, 1, 2, 3, 1, 1, 4], np.int32)
        inv = fo.inverse_pose(Rt)
        return clouds, f1, f2, np.stack([Rt, inv, Rt, inv, Rt, Rt, Rt, inv]), fo.WALL_RADIUS
    f1, f2 = np.array([0, 0, 0, 0, 2, 4], np.int32), np.array([1, 1, 4, 4, 1, 0], np.int32)
    up, down = fo.far_pose(Rt, 50.0), fo.far_pose(Rt, -50.0)
    return clouds, f1, f2, np.stack([up, down, up, down, down, up]), fo.WALL_RADIUS


def overlap_host(name):
    from usip_amd import fragments as fr
    clouds, f1, f2, G, radius = overlap_case(name)
    ratio, hits = fr.overlap_ratio_cpu(fr.host_bank(clouds), f1, f2, G, radius, num_threads=THREADS)
    return dict(ratio=bits(ratio), hits=hits)


def overlap_device(name, dev="cuda:0"):
    import torch
    from usip_amd import fragments as fr
    clouds, f1, f2, G, radius = overlap_case(name)
    ratio, hits = fr.overlap_ratio(fr.FragmentBank(clouds, dev), *(torch.from_numpy(a).to(dev) for a in (f1, f2, G)), radius)
    return dict(ratio=bits(ratio.cpu().numpy()), hits=hits.cpu().numpy())


# ------------------------------------------------------------------------------------------------ trimmed ICP
def icp_case(name):
    """-> (HostBank [A, B], frag1, frag2, Rt0 f64 [1,3,4], mask u8 [1], refine's keywords)"""
    import icp_oracle as io
    from usip_amd import fragments as fr
    f = io.fixture(name)
    return (fr.host_bank([f["A"], f["B"]]), np.array([0], np.int32), np.array([1], np.int32), f["Rt0"][None].copy(),
            np.array([f["mask"]], np.uint8), dict(f["args"]))


def _icp_out(idx, d2, res, cut_d2, cut_i):
    out = dict(nearest_idx=idx, nearest_d2=d2, cut_d2=cut_d2, cut_i=cut_i, **res)
    return {k: bits(v) for k, v in out.items()}


def icp_host(name):
    from usip_amd import fragments as fr
    bank, f1, f2, Rt0, mask, args = icp_case(name)
    idx, d2 = fr.icp_nearest_cpu(bank, f1, f2, Rt0, mask, fr.moved_x_order_cpu(bank, f2, Rt0), THREADS)
    res, cut_d2, cut_i = fr.icp_refine_cpu(bank, f1, f2, Rt0, mask, num_threads=THREADS, want_cuts=True, **args)
    return _icp_out(idx, d2, res._asdict(), cut_d2, cut_i)


def icp_device(name, dev="cuda:0"):
    import torch
    from usip_amd import fragments as fr
    from usip_amd import ops
    bank, f1, f2, Rt0, mask, args = icp_case(name)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)    # noqa: E731
    fine = type("Bank", (), dict(rows=d(bank.rows), offsets=d(bank.offsets), perm=d(bank.perm), lmax=bank.lmax))
    order2 = d(fr.moved_x_order_cpu(bank, f2, Rt0))
    idx, d2 = ops.icp_nearest(fine.rows, fine.offsets, fine.perm, d(f1), d(f2), d(Rt0), bank.lmax, d(mask), order2)
    res, cut_d2, cut_i = fr.icp_refine(fine, d(f1), d(f2), d(Rt0), d(mask), want_cuts=True, **args)
    return _icp_out(idx.cpu().numpy(), d2.cpu().numpy(), {k: v.cpu().numpy() for k, v in res._asdict().items()},
                    cut_d2.cpu().numpy(), cut_i.cpu().numpy())


# ------------------------------------------------------------------------------------------------ scan K nearest
@functools.lru_cache(maxsize=None)
def scan(name):
    n = SCANS[name]
    s = np.random.default_rng(500 + n).normal(size=(n, 4)).astype(np.float32)
    s[n // 2:, :3] = np.round(s[n // 2:, :3] * 2) / 2
    if name.endswith("constant_x"):
        s[:, 0] = np.float32(1.25)
    return s


def knn_host(name, k):
    from usip_amd import prepare
    return prepare.knn_cpu(scan(name), k, num_threads=THREADS)


def knn_device(name, k, dev="cuda:0"):
    import torch
    from usip_amd import prepare
    return prepare.ScanPreparer(dev, k=k).neighbours(torch.from_numpy(scan(name)).to(dev)).cpu().numpy()


# ------------------------------------------------------------------------------------------------ the per-pair pipeline
@functools.lru_cache(maxsize=None)
def scene():
    """-> (sc, args of register_pairs_cpu up to pair_ids with the HostBank left out, clouds)"""
    from usip_amd import fragments as fr
    sc = fr.synthetic_scene(**SCENE)
    F, M = len(sc["clouds"]), max(len(x) for x in sc["xyz"])
    kp, de, cnt = np.zeros((F, 3, M), np.float32), np.zeros((F, SCENE["dim"], M), np.float32), np.zeros(F, np.int32)
    for i in range(F):
        n = len(sc["xyz"][i])
        kp[i, :, :n], de[i, :, :n], cnt[i] = sc["xyz"][i].T, sc["desc"][i].T, n
    pairs = [(a, b) for a in range(F) for b in range(a + 1, F)]
    f1, f2 = np.array([p[0] for p in pairs], np.int32), np.array([p[1] for p in pairs], np.int32)
    return sc, (kp[f1], de[f1], cnt[f1], kp[f2], de[f2], cnt[f2]), (f1, f2, np.arange(len(f1), dtype=np.int64))


def pairs_host(registrator):
    from usip_amd import fragments as fr
    from usip_amd import posegraph as pg
    sc, stacked, (f1, f2, ids) = scene()
    out = fr.register_pairs_cpu(*stacked, fr.host_bank(sc["clouds"]), f1, f2, ids, num_threads=THREADS,
                                registrator=registrator, refine=fr.refine_bank_cpu(sc["clouds"]),
                                dense_radius=pg.INFORMATION_RADIUS)
    return {k: bits(v) for k, v in out.items()}


def pairs_device(registrator, dev="cuda:0"):
    import torch
    from usip_amd import fragments as fr
    from usip_amd import posegraph as pg
    sc, stacked, tail = scene()
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)    # noqa: E731
    out = fr.register_pairs(*(d(a) for a in stacked), fr.FragmentBank(sc["clouds"], dev), *(d(a) for a in tail),
                            registrator=registrator, refine=fr.RefineBank(sc["clouds"], dev),
                            dense_radius=pg.INFORMATION_RADIUS)
    return {k: bits(v.cpu().numpy()) for k, v in out.items()}


# ------------------------------------------------------------------------------------------------ the fixture
def digests():
    import icp_oracle as io
    out = {}
    for name in OVERLAP:
        clouds, f1, f2, G, _ = overlap_case(name)
        out[key("overlap-" + name, "sha256")] = sha(list(clouds) + [f1, f2, G])
    for name in io.NAMES:
        bank, _, _, Rt0, mask, _ = icp_case(name)
        out[key("icp-" + name, "sha256")] = sha([bank.rows, bank.offsets, Rt0, mask])
    for name in SCANS:
        out[key("knn-" + name, "sha256")] = sha([scan(name)])
    sc, stacked, tail = scene()
    out[key("pairs", "sha256")] = sha(list(sc["clouds"]) + list(stacked) + list(tail))
    return out


def key(case, field):
    return "%s__%s" % (case, field)


_PINNED = {}


def check(case, got, what):
    """Every stored output of `case` ("overlap-walls", "icp-lattice", "knn-257", "pairs-fgr") against got {field: stored
    form}, bit for bit; the inputs' digest first (nothing is skipped when a generator moves)."""
    if not _PINNED:
        _PINNED.update(np.load(PATH))
        _PINNED["_digests"] = digests()
    sha = key("pairs" if case.startswith("pairs-") else case, "sha256")
    assert bytes(_PINNED[sha]) == bytes(_PINNED["_digests"][sha]), "the generators no longer give the fixture's inputs: " + case
    stored = {k[len(key(case, "")):]: v for k, v in _PINNED.items() if k.startswith(key(case, "")) and k != sha}
    assert stored and set(stored) == set(got), (case, sorted(stored), sorted(got))
    differ = {k: int((got[k] != e).sum()) if got[k].shape == e.shape else -1 for k, e in stored.items()}
    print("%s, %s: entries that differ from the pinned bits %s" % (what, case, differ))
    for k, e in stored.items():
        assert got[k].dtype == e.dtype and got[k].shape == e.shape, (case, k, got[k].dtype, e.dtype, got[k].shape, e.shape)
        assert np.array_equal(got[k], e), (what, case, k, differ[k])


def main():
    import icp_oracle as io
    out = digests()
    for name in OVERLAP:
        got = overlap_host(name)
        print("overlap", name, "hits", got["hits"].tolist())
        for k, v in got.items():
            out[key("overlap-" + name, k)] = v
    for name in io.NAMES:
        got = icp_host(name)
        print("icp", name, "iterations", got["iterations"].tolist(), "hits", got["hits"].tolist(), "cut_i", got["cut_i"].tolist())
        for k, v in got.items():
            out[key("icp-" + name, k)] = v
    for name in SCANS:
        for k in KNN_K:
            out[key("knn-" + name, "idx%d" % k)] = knn_host(name, k)
        print("knn", name, "idx1[:4]", out[key("knn-" + name, "idx1")][:4, 0].tolist())
    for reg in REGISTRATORS:
        got = pairs_host(reg)
        print("pairs", reg, "inliers", got["inliers"].tolist(), "gate_refined", got["gate_refined"].tolist(), "dense_count",
              got["dense_count"].tolist())
        for k, v in got.items():
            out[key("pairs-" + reg, k)] = v
    np.savez_compressed(PATH, **out)
    size = os.path.getsize(PATH)
    print("wrote", PATH, "%.0f KB" % (size / 1024))
    if size >= os.path.getsize(os.path.join(HERE, "cloud_stage_parent_bits.npz")):
        raise SystemExit("the fixture is not smaller than cloud_stage_parent_bits.npz")


if __name__ == "__main__":
    main()
