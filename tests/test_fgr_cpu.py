"""The f-12 host twin (csrc/fgr_cpu.cpp over csrc/fgr_math.h) against the numpy restatement of the contract
(tests/fgr_oracle.py), on the smallest shapes at which each mechanism can go wrong.  tests/test_fgr_gpu.py then holds the
device to this twin bit for bit.

Integers (mutual rows, accepted rows, row_count, trials_walked, valid, the inlier mask) must be equal; each fixture first
asserts that no decision behind them hangs on rounding: no edge ratio within 1e-9 of 0.95 or 1 / 0.95, no residual within
1e-9 of the threshold.  Rt: the oracle run with its rows forward and reversed differs from itself by its own summation
noise (measured over these fixtures: at most 8.9e-16); the twin, whose expression order differs from numpy's in the same
way, may be 1000 times that away, and that allowance must itself stay below 1e-9 (error met: at most 1.8e-15)."""
import ctypes

import numpy as np
import pytest

import fgr_oracle as fo
from usip_amd import _lib
from usip_amd import fragments as fr

MARGIN = 1e-9
SINCOS_BOUND = 2.3e-16      # csrc/fgr_math.h: fgr_sincos


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def batch(names, clip=True):
    """the fixtures stacked into one ragged call, padded to the widest: (kp1, kp2, n1, n2, nn12, nn21, triples)"""
    fx = [fo.fixture(n) for n in names]
    M, T = max(f["kp1"].shape[1] for f in fx), max(len(f["triples"]) for f in fx)
    P = len(fx)
    kp1, kp2 = np.zeros((P, 3, M), np.float32), np.zeros((P, 3, M), np.float32)
    nn12, nn21 = np.zeros((P, M), np.int32), np.zeros((P, M), np.int32)
    n1, n2, triples = np.zeros(P, np.int32), np.zeros(P, np.int32), np.zeros((P, T, 3), np.int32)
    for p, f in enumerate(fx):
        m = f["kp1"].shape[1]
        kp1[p, :, :m], kp2[p, :, :m], nn12[p, :m], nn21[p, :m] = f["kp1"], f["kp2"], f["nn12"], f["nn21"]
        n1[p], n2[p] = (np.clip(f["n1"], 0, m), np.clip(f["n2"], 0, m)) if clip and P > 1 else (f["n1"], f["n2"])
        triples[p, :len(f["triples"])] = f["triples"]
    return kp1, kp2, n1, n2, nn12, nn21, triples


def twin(names, **kw):
    kp1, kp2, n1, n2, nn12, nn21, triples = batch(names)
    return fr.fgr_registration_cpu(kp1, kp2, n1, n2, nn12, nn21, triples=triples, **kw)


def allowance():
    noise = fo.noise()
    print("oracle noise %.3e, allowance %.3e" % (noise, 1000 * noise))
    assert 0 < 1000 * noise < 1e-9
    return 1000 * noise


def against_oracle(r, p, name, allow):
    """pair p of the result r against the oracle's result of fixture `name`"""
    f = fo.fixture(name)
    o = f["oracle"]
    assert o["edge_margin"] > MARGIN and o["residual_margin"] > MARGIN, (name, o["edge_margin"], o["residual_margin"])
    nc, nr = o["nc"], o["row_count"]
    assert int(r.counts[p]) == nc and np.array_equal(r.mutual[p, :nc], o["mutual"]) and not r.mutual[p, nc:].any(), name
    assert int(r.row_count[p]) == nr and np.array_equal(r.rows[p, :nr], o["rows"]) and not r.rows[p, nr:].any(), name
    assert int(r.trials_walked[p]) == o["trials_walked"], (name, int(r.trials_walked[p]), o["trials_walked"])
    assert int(r.valid[p]) == o["valid"], name
    err = float(np.abs(r.Rt[p] - o["Rt"]).max())
    print("%s: nc %d, rows %d, walked %d of %d, | Rt - oracle | %.3e" % (name, nc, nr, o["trials_walked"], o["T"], err))
    assert err <= allow, (name, err, allow)
    m = len(o["inlier_mask"])
    assert np.array_equal(r.inlier_mask[p, :m], o["inlier_mask"]) and not r.inlier_mask[p, m:].any(), name
    assert int(r.inliers[p]) == o["inliers"] and r.inlier_ratio[p] == o["inliers"] / max(nc, 1), name
    if not o["valid"]:
        assert bits(r.Rt[p]).tolist() == bits(np.eye(3, 4)).tolist() and int(r.inliers[p]) == 0, name


def same_result(a, b, pa=slice(None), pb=slice(None), width=None):
    for name in fr.FgrResult._fields:
        x, y = getattr(a, name), getattr(b, name)
        if x is None:
            assert y is None, name
            continue
        x, y = np.asarray(x)[pa], np.asarray(y)[pb]
        if width is not None and name in ("mutual", "inlier_mask"):
            assert not x[:, width:].any() and not y[:, width:].any(), name
            x, y = x[:, :width], y[:, :width]
        assert x.dtype == y.dtype and x.shape == y.shape, name
        assert np.array_equal(bits(x), bits(y)), name


@pytest.mark.parametrize("name", fo.NAMES)
def test_fixture_equals_the_oracle(name):
    against_oracle(twin([name]), 0, name, allowance())


def test_identical_fragments_give_the_identity():
    r, allow = twin(["identical"]), allowance()
    assert int(r.valid[0]) == 1 and np.abs(r.Rt[0] - np.eye(3, 4)).max() <= allow


def test_counts_outside_the_range_behave_as_the_ends():
    kp1, kp2, n1, n2, nn12, nn21, triples = batch(["cap"])
    ref = fr.fgr_registration_cpu(kp1, kp2, n1, n2, nn12, nn21, triples=triples)
    big = fr.fgr_registration_cpu(kp1, kp2, [2 ** 31 - 1], [65], nn12, nn21, triples=triples)
    same_result(ref, big)
    none = fr.fgr_registration_cpu(kp1, kp2, n1, [-3], nn12, nn21, triples=triples)
    assert int(none.counts[0]) == 0 and int(none.valid[0]) == 0 and int(none.trials_walked[0]) == 0
    assert not none.mutual.any() and not none.inlier_mask.any()


def test_ragged_batch_equals_every_pair_alone():
    names = [n for n in fo.NAMES if n != "counts_beyond"]
    allow = allowance()
    whole = twin(names, num_threads=4)
    for p, name in enumerate(names):
        against_oracle(whole, p, name, allow)
        same_result(whole, twin([name]), slice(p, p + 1), width=fo.fixture(name)["kp1"].shape[1])


def test_sincos_against_numpy_on_a_dense_grid():
    x = np.linspace(-np.pi, np.pi, 2000001)
    assert x[0] == -np.pi and x[-1] == np.pi
    s, c = np.zeros_like(x), np.zeros_like(x)
    _lib.check(_lib.lib().usip_fgr_sincos_f64_cpu(ctypes.c_void_p(x.ctypes.data), len(x), ctypes.c_void_p(s.ctypes.data),
                                                  ctypes.c_void_p(c.ctypes.data)), "usip_fgr_sincos_f64_cpu")
    es, ec = float(np.abs(s - np.sin(x)).max()), float(np.abs(c - np.cos(x)).max())
    print("fgr_sincos against numpy: sin %.3e, cos %.3e" % (es, ec))
    assert es <= SINCOS_BOUND and ec <= SINCOS_BOUND
    assert (np.abs(s) <= 1).all() and (np.abs(c) <= 1).all() and np.abs(s * s + c * c - 1).max() <= 4 * SINCOS_BOUND


PHILOX = ["cap", "sparse", "few_rows", "unrelated", "nc2", "coincident"]


def philox(order, seed=7, ids=None, **kw):
    kp1, kp2, n1, n2, nn12, nn21, _ = batch(PHILOX)
    o = np.asarray(order)
    t = fr.fgr_tuples_cpu(kp1[o], kp2[o], n1[o], n2[o], nn12[o], nn21[o], seed, ids, None, **kw)
    return t, fr.fgr_registration_cpu(kp1[o], kp2[o], n1[o], n2[o], nn12[o], nn21[o], seed=seed, pair_ids=ids)


def test_philox_triples_are_distinct_in_range_and_reproducible():
    order = np.arange(len(PHILOX))
    t, r = philox(order, want_triples=4000)
    t2, r2 = philox(order, want_triples=4000, num_threads=3)
    same_result(r, r2)
    assert np.array_equal(t["triples"], t2["triples"])
    assert int(r.valid[0]) == 1 and int(r.row_count[0]) == 3000 and int(r.valid[1]) == 1       # cap and sparse register
    for p in range(len(PHILOX)):
        nc, walked = int(t["mutual_count"][p]), int(t["trials_walked"][p])
        tr = t["triples"][p, :min(walked, 4000)]
        assert not t["triples"][p, walked:].any()
        if PHILOX[p] == "coincident":
            assert walked == 0
        elif nc >= 3:
            assert walked > 0 and tr.min() >= 0 and tr.max() < nc
            assert ((tr[:, 0] != tr[:, 1]) & (tr[:, 0] != tr[:, 2]) & (tr[:, 1] != tr[:, 2])).all()
            assert len(np.unique(tr, axis=0)) > len(tr) // 2                                     # and they do vary
    other, _ = philox(order, seed=8, want_triples=4000)
    assert not np.array_equal(other["triples"][0], t["triples"][0])
    # the drawn triples, handed back as explicit ones, give the same rows
    kp1, kp2, n1, n2, nn12, nn21, _ = batch(PHILOX)
    back = fr.fgr_registration_cpu(kp1, kp2, n1, n2, nn12, nn21, triples=t["triples"])
    same_result(r, back)


def test_a_batch_permuted_with_its_pair_ids_gives_the_same_pairs():
    n = len(PHILOX)
    ids = np.arange(100, 100 + n, dtype=np.int64)
    _, r = philox(np.arange(n), ids=ids)
    perm = np.array([3, 0, 5, 1, 4, 2])
    _, q = philox(perm, ids=ids[perm])
    for k, p in enumerate(perm):
        same_result(q, r, slice(k, k + 1), slice(p, p + 1))
    _, plain = philox(np.arange(n))                                    # NULL ids: the pair's own position
    same_result(plain, philox(np.arange(n), ids=np.arange(n, dtype=np.int64))[1])
    assert not np.array_equal(plain.rows[0], r.rows[0])


def test_shapes_outside_the_limits_are_refused():
    kp = np.zeros((1, 3, 1025), np.float32)
    z = np.zeros((1, 1025), np.int32)
    with pytest.raises(RuntimeError):
        fr.fgr_registration_cpu(kp, kp, [0], [0], z, z)
    lib = _lib.lib()
    p = ctypes.c_void_p(kp.ctypes.data)
    assert lib.usip_fgr_tuples_f32_cpu(p, p, p, p, p, p, 1, 1025, 0, None, None, 0, p, p, p, p, p, p, None, 0, 1) < 0
    assert lib.usip_fgr_tuples_f32_cpu(p, p, p, p, p, p, 65536, 16, 0, None, None, 0, p, p, p, p, p, p, None, 0, 1) < 0
    assert lib.usip_fgr_tuples_f32_cpu(p, p, p, p, p, p, 1, 16, 0, None, None, 0, None, p, p, p, p, p, None, 0, 1) < 0
    assert lib.usip_fgr_tuples_explicit_f32_cpu(p, p, p, p, p, p, 1, 16, None, 5, p, p, p, p, p, p, 1) < 0
    assert lib.usip_fgr_optimize_f32_cpu(p, p, p, p, p, p, p, 1, 0, 0.2, p, p, p, p, 1) < 0
    assert lib.usip_fgr_optimize_f32_cpu(p, p, p, p, p, p, p, 0, 16, 0.2, p, p, p, p, 1) == 0


def scene_arrays(sc, top):
    F, D = len(sc["xyz"]), sc["desc"][0].shape[1]
    kp, de, cnt = np.zeros((F, 3, top), np.float32), np.zeros((F, D, top), np.float32), np.zeros(F, np.int32)
    for i in range(F):
        n = len(sc["xyz"][i])
        kp[i, :, :n], de[i, :, :n], cnt[i] = sc["xyz"][i].T, sc["desc"][i].T, n
    pairs = [(i, j) for i in range(F) for j in range(i + 1, F)]
    return kp, de, cnt, np.array([p[0] for p in pairs], np.int32), np.array([p[1] for p in pairs], np.int32)


def test_synthetic_scene_is_recovered_by_fgr_through_the_host_twins():
    sc = fr.synthetic_scene(0, 6, 4000)
    kp, de, cnt, f1, f2 = scene_arrays(sc, 128)
    o = fr.register_pairs_cpu(kp[f1], de[f1], cnt[f1], kp[f2], de[f2], cnt[f2], fr.host_bank(sc["clouds"]), f1, f2,
                              np.arange(len(f1)), num_threads=8, registrator="fgr")
    assert set(o) == {"Rt", "inliers", "inlier_ratio", "valid", "matches", "row_count", "trials_walked", "information",
                      "ratio_aligned", "overlap_hits", "gate", "frag1", "frag2"}
    s = fr.summarize(o, list(range(6)), sc["gt"], sc["gt_info"])
    print("fgr on the synthetic scene: recall %.3f precision %.3f of %d" % (s["recall"], s["precision"], s["gt_num"]))
    assert s["gt_num"] >= 6 and s["recall"] == 1.0
    # a pair the ground truth leaves out (under 30 % overlap) may still register and pass the gate, which evaluate_log
    # counts against precision; what must hold is that every pair written carries the right pose
    assert s["written"] >= s["gt_num"]
    for p in np.nonzero(o["gate"])[0]:
        want = (np.linalg.inv(sc["poses"][f1[p]]) @ sc["poses"][f2[p]])[:3]
        assert o["valid"][p] and np.abs(o["Rt"][p] - want).max() < 1e-5, (f1[p], f2[p])


def test_ransac_through_the_new_argument_is_the_call_without_it():
    sc = fr.synthetic_scene(0, 4, 2000)
    kp, de, cnt, f1, f2 = scene_arrays(sc, 128)
    args = (kp[f1], de[f1], cnt[f1], kp[f2], de[f2], cnt[f2], fr.host_bank(sc["clouds"]), f1, f2, np.arange(len(f1)))
    a = fr.register_pairs_cpu(*args, max_trials=300, num_threads=4)
    b = fr.register_pairs_cpu(*args, max_trials=300, num_threads=4, registrator="ransac")
    assert list(a) == list(b)
    for k in a:
        assert np.array_equal(bits(a[k]), bits(b[k])), k
    with pytest.raises(ValueError):
        fr.register_pairs_cpu(*args, registrator="icp")
